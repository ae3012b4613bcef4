// Launcher interface of the optimizer step (optim_kernels.hip): the AdamW update of torch.optim.AdamW (decoupled weight decay,
// non-amsgrad, non-maximize) over a LIST of parameter tensors, the 2-norm of a list of gradients, and the clip of
// torch.nn.utils.clip_grad_norm_.  One family of multi-tensor kernels after gan_loss_launch.h: a launch covers up to
// kOptimMaxTensors list entries whose table (pointers, element counts, first block) travels by value as a kernel argument --
// no device allocation, no table copy.  fp32 in and out.  The update is elementwise with explicitly rounded operations: an
// element's new p, m, v depend on nothing but its own p, g, m, v and the entry's scalars, whatever block, lane or access width
// handled it.  The norm accumulates in fp64 in one fixed order (per thread ascending, then a fixed tree, no atomics).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace st {

constexpr int kOptimMaxTensors = 64;        // list entries per launch: 64 x 56 B (update) / 24 B (norm, clip) of kernel argument
constexpr int kOptimChunk = 4096;           // elements of one entry a block works on: 256 threads x 4 groups of 4

struct AdamwEntry {           // one list entry of an update launch
    float* p;
    const float* g;
    float* m;                 // exp_avg
    float* v;                 // exp_avg_sq
    long long n;              // elements, >= 1
    int first_block;          // index of the entry's first chunk in the launch's grid (ascending over the table)
    float step_size;          // lr / (1 - beta1^step), from the host's double
    float bc2_sqrt;           // sqrt(1 - beta2^step)
    int pad;
};
struct AdamwTable { AdamwEntry e[kOptimMaxTensors]; };

struct AdamwScalars {         // the group's constants, rounded from the host's doubles
    float decay;              // 1 - lr * weight_decay
    float one_minus_beta1;
    float beta2;
    float one_minus_beta2;
    float eps;
};

struct GradEntry {            // one list entry of a norm or clip launch
    float* g;
    long long n;
    int first_block;
    int pad;
};
struct GradTable { GradEntry e[kOptimMaxTensors]; };

// chunks of an entry of n elements (= its blocks in a launch, its fp64 partials in the norm's scratch)
inline long long optim_chunks(long long n) { return (n + kOptimChunk - 1) / kOptimChunk; }

// One launch group: n <= kOptimMaxTensors entries whose first_block fields are filled and sum to `blocks`.
hipError_t launch_adamw_step(const AdamwTable& tab, int n, int blocks, const AdamwScalars& sc, hipStream_t s);
// partials: `blocks` doubles of scratch of this group, one squared sum per chunk
hipError_t launch_grad_sumsq(const GradTable& tab, int n, int blocks, double* partials, hipStream_t s);
// total_norm[0] = (float)sqrt(sum of the n_partials partials: per thread ascending, then the tree); n_partials == 0 writes 0
hipError_t launch_grad_norm_finish(const double* partials, long long n_partials, float* total_norm, hipStream_t s);
// g *= min(max_norm / (total_norm[0] + 1e-6f), 1.0f), read on the device; a coefficient of exactly 1.0f touches no gradient
hipError_t launch_grad_clip(const GradTable& tab, int n, int blocks, const float* total_norm, float max_norm, hipStream_t s);

}  // namespace st
