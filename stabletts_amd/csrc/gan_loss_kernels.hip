// The three scalar GAN losses of a Vocos step (vocoders/vocos/models/loss.py:37-66) and their gradients as multi-tensor
// kernels: one launch covers up to kGanLossMaxPairs list entries, the table of which is a kernel argument.  HBM-bound, fp32
// element ops, no MFMA.  Every sum is fp64 in one fixed order (per thread ascending, then block_sum_f64's tree); no atomics.
//
// Which elements a thread sums is fixed by the element's index INSIDE ITS ENTRY alone: chunk = index / kGanLossChunk, and inside
// a chunk group q = 4 consecutive elements goes to thread q % 256 as its (q / 256)-th group.  Nothing depends on where the entry
// starts in memory, so an entry that is the second half of a larger tensor (4-byte aligned only) sums in the same order as the
// same values in a tensor of their own, and the two give the same bits.  That rules out peeling a scalar head up to a 16-byte
// boundary (it would shift every later group); instead a whole group is ONE 16-byte load through a vector type of 4-byte
// alignment -- global_load_dwordx4 needs dword alignment only -- and only an entry's last, partial group is read by scalars.
#include "common.h"
#include "block_reduce.h"
#include "gan_loss_launch.h"

namespace st {

namespace {

typedef float gan_f4 __attribute__((ext_vector_type(4)));
typedef gan_f4 gan_f4_a4 __attribute__((aligned(4)));          // four floats at any float address

constexpr int kGroupsPerThread = kGanLossChunk / (256 * 4);
static_assert(kGroupsPerThread * 256 * 4 == kGanLossChunk, "a chunk is a whole number of 256 x 4 element rounds");
static_assert(kGanLossMaxPairs % 2 == 0, "GAN_OP_ALTERNATE reads an entry's parity from its index in the launch");
static_assert(sizeof(GanPairTable) <= 2048 && sizeof(GanGradTable) <= 3072, "the tables travel as kernel arguments (4 KB in all)");

__device__ __forceinline__ gan_f4 load4(const float* p) { return *(const gan_f4_a4*)p; }
__device__ __forceinline__ void store4(float* p, gan_f4 v) { *(gan_f4_a4*)p = v; }

// entry of block blk: the last one whose first_block <= blk (first_block ascends, p[0].first_block == 0)
template <class Table>
__device__ __forceinline__ int find_entry(const Table& tab, int n_pairs, int blk) {
    int lo = 0, hi = n_pairs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab.p[mid].first_block <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one element's term, fp32 op and an exact fp64 square
template <int OP>
__device__ __forceinline__ double gan_term(float a, float b, bool odd) {
    if (OP == GAN_OP_ABS_DIFF) return (double)fabsf(a - b);
    if (OP == GAN_OP_ONE_MINUS_SQ || (OP == GAN_OP_ALTERNATE && !odd)) { const float d = 1.0f - a; return (double)d * (double)d; }
    return (double)a * (double)a;
}

}  // namespace

// Stage 1.  One block: one chunk of one entry -> one fp64 partial.
template <int OP>
__global__ __launch_bounds__(256) void gan_loss_partial_kernel(const GanPairTable tab, int n_pairs, double* partials) {
    __shared__ double red[256];
    constexpr bool two = OP == GAN_OP_ABS_DIFF;
    const int blk = blockIdx.x;
    const int ent = find_entry(tab, n_pairs, blk);
    const long long start = (long long)(blk - tab.p[ent].first_block) * kGanLossChunk;
    const long long left = tab.p[ent].n - start;
    const int len = left < (long long)kGanLossChunk ? (int)left : kGanLossChunk;       // >= 1
    const float* a = tab.p[ent].a + start;
    const float* b = two ? tab.p[ent].b + start : a;
    const bool odd = ent & 1;
    double acc = 0.0;
    if (len == kGanLossChunk) {                // a full chunk: every load issued before the first add
        gan_f4 va[kGroupsPerThread], vb[kGroupsPerThread];
#pragma unroll
        for (int k = 0; k < kGroupsPerThread; ++k) {
            const int g = (k * 256 + (int)threadIdx.x) * 4;
            va[k] = load4(a + g);
            vb[k] = two ? load4(b + g) : va[k];
        }
#pragma unroll
        for (int k = 0; k < kGroupsPerThread; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += gan_term<OP>(va[k][j], vb[k][j], odd);
    } else {                                   // the entry's last chunk: whole groups as above, the last one by scalars
        for (int k = 0; k < kGroupsPerThread; ++k) {
            const int g = (k * 256 + (int)threadIdx.x) * 4;
            if (g + 4 <= len) {
                const gan_f4 va = load4(a + g), vb = two ? load4(b + g) : va;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc += gan_term<OP>(va[j], vb[j], odd);
            } else {
                for (int j = g; j < len; ++j) acc += gan_term<OP>(a[j], b[j], odd);
            }
        }
    }
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) partials[blk] = acc;
}

// Stage 2.  One block per entry: its partials, ascending per thread, then the tree; mean = sum / n.
__global__ __launch_bounds__(256) void gan_loss_mean_kernel(const GanPairTable tab, int n_pairs, int blocks, const double* partials,
                                                            double* means64, float* out_means) {
    __shared__ double red[256];
    const int ent = blockIdx.x;
    const int first = tab.p[ent].first_block, last = ent + 1 < n_pairs ? tab.p[ent + 1].first_block : blocks;
    double acc = 0.0;
    for (int i = first + (int)threadIdx.x; i < last; i += 256) acc += partials[i];
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) {
        const double mean = acc / (double)tab.p[ent].n;
        means64[ent] = mean;
        out_means[ent] = (float)mean;
    }
}

// Stage 3.  The means in list order, fp64, times the scale.
__global__ __launch_bounds__(256) void gan_loss_total_kernel(const double* means64, int n, float scale, float* out) {
    __shared__ double buf[256];
    double acc = 0.0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + (int)threadIdx.x;
        __syncthreads();
        buf[threadIdx.x] = i < n ? means64[i] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = n - base < 256 ? n - base : 256;
            for (int j = 0; j < m; ++j) acc += buf[j];
        }
    }
    if (threadIdx.x == 0) out[0] = (float)(acc * (double)scale);
}

template <int OP>
static hipError_t launch_partial(const GanPairTable& tab, int n_pairs, int blocks, double* partials, hipStream_t s) {
    hipLaunchKernelGGL(gan_loss_partial_kernel<OP>, dim3(blocks), dim3(256), 0, s, tab, n_pairs, partials);
    return hipGetLastError();
}

hipError_t launch_gan_loss_group(int op, const GanPairTable& tab, int n_pairs, int blocks, double* partials, double* means64,
                                 float* out_means, hipStream_t s) {
    if (n_pairs < 1 || n_pairs > kGanLossMaxPairs || blocks < n_pairs) return hipErrorInvalidValue;
    hipError_t rc;
    switch (op) {
        case GAN_OP_ABS_DIFF: rc = launch_partial<GAN_OP_ABS_DIFF>(tab, n_pairs, blocks, partials, s); break;
        case GAN_OP_ONE_MINUS_SQ: rc = launch_partial<GAN_OP_ONE_MINUS_SQ>(tab, n_pairs, blocks, partials, s); break;
        case GAN_OP_SQ: rc = launch_partial<GAN_OP_SQ>(tab, n_pairs, blocks, partials, s); break;
        case GAN_OP_ALTERNATE: rc = launch_partial<GAN_OP_ALTERNATE>(tab, n_pairs, blocks, partials, s); break;
        default: return hipErrorInvalidValue;
    }
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(gan_loss_mean_kernel, dim3(n_pairs), dim3(256), 0, s, tab, n_pairs, blocks, partials, means64, out_means);
    return hipGetLastError();
}

hipError_t launch_gan_loss_total(const double* means64, int n, float scale, float* out, hipStream_t s) {
    hipLaunchKernelGGL(gan_loss_total_kernel, dim3(1), dim3(256), 0, s, means64, n, scale, out);
    return hipGetLastError();
}

// Backward.  One block: one chunk of one entry, recomputed from the saved inputs; whole groups by 16-byte loads and stores, the
// entry's last partial group by scalars.
template <int OP>
__global__ __launch_bounds__(256) void gan_loss_backward_kernel(const GanGradTable tab, int n_pairs, const float* gout) {
    constexpr bool two = OP == GAN_OP_ABS_DIFF;
    const int blk = blockIdx.x;
    const int ent = find_entry(tab, n_pairs, blk);
    const long long start = (long long)(blk - tab.p[ent].first_block) * kGanLossChunk;
    const long long left = tab.p[ent].n - start;
    const int len = left < (long long)kGanLossChunk ? (int)left : kGanLossChunk;
    const float* a = tab.p[ent].a + start;
    const float* b = two ? tab.p[ent].b + start : a;
    float* da = tab.p[ent].da ? tab.p[ent].da + start : nullptr;
    float* db = two && tab.p[ent].db ? tab.p[ent].db + start : nullptr;
    const double s64 = (double)gout[0] * 2.0 / (double)tab.p[ent].n;
    const float s = (float)s64;
    const bool sq = OP == GAN_OP_SQ || (OP == GAN_OP_ALTERNATE && (ent & 1));
    auto grad = [&](float x, float y) -> float {        // d / d a of the entry's mean, times gout
        if (two) return x > y ? s : (x < y ? -s : 0.0f);                       // s sign(r - g), sign(0) = 0
        return (float)(s64 * (sq ? (double)x : (double)x - 1.0));
    };
#pragma unroll 2
    for (int k = 0; k < kGroupsPerThread; ++k) {
        const int g = (k * 256 + (int)threadIdx.x) * 4;
        if (g + 4 <= len) {
            const gan_f4 va = load4(a + g), vb = two ? load4(b + g) : va;
            gan_f4 ga;
#pragma unroll
            for (int j = 0; j < 4; ++j) ga[j] = grad(va[j], vb[j]);
            if (da) store4(da + g, ga);
            if (db) store4(db + g, -ga);
        } else {
            for (int j = g; j < len; ++j) {
                const float v = grad(a[j], b[j]);
                if (da) da[j] = v;
                if (db) db[j] = -v;
            }
        }
    }
}

hipError_t launch_gan_loss_backward_group(int op, const GanGradTable& tab, int n_pairs, int blocks, const float* gout, hipStream_t s) {
    if (n_pairs < 1 || n_pairs > kGanLossMaxPairs || blocks < n_pairs) return hipErrorInvalidValue;
    switch (op) {
        case GAN_OP_ABS_DIFF: hipLaunchKernelGGL(gan_loss_backward_kernel<GAN_OP_ABS_DIFF>, dim3(blocks), dim3(256), 0, s, tab, n_pairs, gout); break;
        case GAN_OP_ONE_MINUS_SQ: hipLaunchKernelGGL(gan_loss_backward_kernel<GAN_OP_ONE_MINUS_SQ>, dim3(blocks), dim3(256), 0, s, tab, n_pairs, gout); break;
        case GAN_OP_SQ: hipLaunchKernelGGL(gan_loss_backward_kernel<GAN_OP_SQ>, dim3(blocks), dim3(256), 0, s, tab, n_pairs, gout); break;
        case GAN_OP_ALTERNATE: hipLaunchKernelGGL(gan_loss_backward_kernel<GAN_OP_ALTERNATE>, dim3(blocks), dim3(256), 0, s, tab, n_pairs, gout); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace st
