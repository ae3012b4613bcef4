// Launcher interface of the three scalar GAN losses of a Vocos step (gan_loss_kernels.hip): feature matching
// sum_i mean|r_i - g_i| * 2 and the two LSGAN terms mean((1 - x)^2), mean(x^2), each over a LIST of tensors of any sizes, and
// their gradients.  One family of multi-tensor kernels: a launch covers up to kGanLossMaxPairs list entries whose table
// (pointers, element counts, first block) travels by value as a kernel argument -- no device allocation, no table copy.
// fp32 in and out; every sum accumulates in fp64 in one fixed order (per thread ascending, then a fixed tree, no atomics), and
// an entry's mean depends on nothing but that entry's values: the same bits alone, at any list position, in any launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace st {

constexpr int kGanLossMaxPairs = 64;        // list entries per launch: 64 x 32 B (forward) / 48 B (backward) of kernel argument
constexpr int kGanLossChunk = 8192;         // elements of one entry a block sums: 256 threads x 8 groups of 4

enum GanLossOp {
    GAN_OP_ABS_DIFF = 0,      // |r - g|                              (feature matching; two inputs)
    GAN_OP_ONE_MINUS_SQ = 1,  // (1 - x)^2
    GAN_OP_SQ = 2,            // x^2
    GAN_OP_ALTERNATE = 3      // (1 - x)^2 for the even list entries, x^2 for the odd ones (discriminator_loss: r0, g0, r1, g1, ...)
};

struct GanPair {              // one list entry of a forward launch
    const float* a;           // r (or x)
    const float* b;           // g (unused by the LSGAN ops)
    long long n;              // elements, >= 1
    int first_block;          // index of the entry's first chunk in the launch's grid (ascending over the table)
    int pad;
};
struct GanPairTable { GanPair p[kGanLossMaxPairs]; };

struct GanGradPair {          // one list entry of a backward launch
    const float* a;
    const float* b;
    float* da;                // nullable: that side gets no gradient
    float* db;
    long long n;
    int first_block;
    int pad;
};
struct GanGradTable { GanGradPair p[kGanLossMaxPairs]; };

// chunks of an entry of n elements (= its blocks in stage 1, its fp64 partials in the scratch)
inline long long gan_loss_chunks(long long n) { return (n + kGanLossChunk - 1) / kGanLossChunk; }

// Stage 1 + 2 of one launch group: n_pairs <= kGanLossMaxPairs entries whose first_block fields are filled and sum to
// `blocks`.  partials: `blocks` doubles of scratch of this group; means64 / out_means: this group's slots (n_pairs each).
hipError_t launch_gan_loss_group(int op, const GanPairTable& tab, int n_pairs, int blocks, double* partials, double* means64,
                                 float* out_means, hipStream_t s);
// Stage 3: out[0] = scale * (sum of the n means in list order, fp64)
hipError_t launch_gan_loss_total(const double* means64, int n, float scale, float* out, hipStream_t s);
// Backward of one launch group (elementwise, plain vector stores), every entry scaled by its own count n:
// feature matching  d g = -gout 2 / n sign(r - g), d r = -d g (sign(0) = 0);  LSGAN  d x = gout 2 (x - 1) / n  or  gout 2 x / n.
// gout: device scalar.  `blocks`: the sum of the entries' chunk counts, as in the forward.
hipError_t launch_gan_loss_backward_group(int op, const GanGradTable& tab, int n_pairs, int blocks, const float* gout, hipStream_t s);

}  // namespace st
