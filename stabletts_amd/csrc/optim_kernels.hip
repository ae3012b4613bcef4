// The optimizer step of both training loops as multi-tensor kernels: the AdamW update, the gradients' 2-norm and the clip of
// clip_grad_norm_.  One launch covers up to kOptimMaxTensors list entries, the table of which is a kernel argument; block b works
// on one kOptimChunk-element chunk of one entry, found from the entry's first_block.  HBM-bound, fp32 element ops, no MFMA.
//
// The update and the clip are elementwise and written with explicitly rounded operations (no contraction, correctly rounded
// division and square root): an element's result is the same bits on the 16-byte path (every pointer of the entry 16-byte
// aligned) and on the scalar path (any float address: views into flat buffers, DDP buckets), in any block and lane.
//
// The norm's squares and sums are fp64 in one fixed order.  Which elements a thread sums is fixed by the element's index INSIDE
// ITS ENTRY alone, as in gan_loss_kernels.hip: group q = 4 consecutive elements of a chunk goes to thread q % 256; a whole group
// is one 16-byte load through a vector type of 4-byte alignment (global_load_dwordx4 needs dword alignment only), so an entry's
// partials do not change with its address.
#include "block_reduce.h"
#include "optim_launch.h"

namespace st {

namespace {

typedef float opt_f4 __attribute__((ext_vector_type(4)));
typedef opt_f4 opt_f4_a4 __attribute__((aligned(4)));          // four floats at any float address

constexpr int kGroupsPerThread = kOptimChunk / (256 * 4);
static_assert(kGroupsPerThread * 256 * 4 == kOptimChunk, "a chunk is a whole number of 256 x 4 element rounds");
static_assert(sizeof(AdamwTable) + sizeof(AdamwScalars) + 16 <= 3840 && sizeof(GradTable) <= 2048,
              "the tables travel as kernel arguments (4 KB in all, hidden arguments included)");

__device__ __forceinline__ opt_f4 load4(const float* p) { return *(const opt_f4*)p; }          // p 16-byte aligned
__device__ __forceinline__ void store4(float* p, opt_f4 v) { *(opt_f4*)p = v; }
__device__ __forceinline__ opt_f4 load4_any(const float* p) { return *(const opt_f4_a4*)p; }

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// entry of block blk: the last one whose first_block <= blk (first_block ascends, e[0].first_block == 0)
template <class Table>
__device__ __forceinline__ int find_entry(const Table& tab, int n, int blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab.e[mid].first_block <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one element of torch.optim.AdamW's update, every operation rounded once to fp32
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const AdamwScalars& sc, float step_size, float bc2_sqrt) {
    p = __fmul_rn(p, sc.decay);                                                                  // p *= 1 - lr wd
    m = __fmaf_rn(__fsub_rn(g, m), sc.one_minus_beta1, m);                                       // m += (g - m)(1 - b1)
    v = __fmaf_rn(__fmul_rn(sc.one_minus_beta2, g), g, __fmul_rn(v, sc.beta2));                  // v = v b2 + (1 - b2) g g
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), bc2_sqrt), sc.eps);
    p = __fsub_rn(p, __fmul_rn(step_size, __fdiv_rn(m, denom)));
}

// the same on a group of four
__device__ __forceinline__ void adamw_group(opt_f4& p, const opt_f4& g, opt_f4& m, opt_f4& v, const AdamwScalars& sc, float step_size,
                                            float bc2_sqrt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float ep = p[j], em = m[j], ev = v[j];
        adamw_elem(ep, g[j], em, ev, sc, step_size, bc2_sqrt);
        p[j] = ep; m[j] = em; v[j] = ev;
    }
}

}  // namespace

__global__ __launch_bounds__(256) void adamw_step_kernel(const AdamwTable tab, int n, const AdamwScalars sc) {
    const int blk = blockIdx.x;
    const int ent = find_entry(tab, n, blk);
    const AdamwEntry& e = tab.e[ent];
    const long long start = (long long)(blk - e.first_block) * kOptimChunk;
    const long long left = e.n - start;
    const int len = left < (long long)kOptimChunk ? (int)left : kOptimChunk;                     // >= 1
    float* p = e.p + start;
    const float* g = e.g + start;
    float* m = e.m + start;
    float* v = e.v + start;
    const float step_size = e.step_size, bc2_sqrt = e.bc2_sqrt;
    // a chunk starts a multiple of 16 bytes into its entry: the entry's alignment is the chunk's
    if (aligned16(e.p) && aligned16(e.g) && aligned16(e.m) && aligned16(e.v)) {
        if (len == kOptimChunk) {              // a full chunk: every load issued before the first use
            opt_f4 vp[kGroupsPerThread], vg[kGroupsPerThread], vm[kGroupsPerThread], vv[kGroupsPerThread];
#pragma unroll
            for (int k = 0; k < kGroupsPerThread; ++k) {
                const int i = (k * 256 + (int)threadIdx.x) * 4;
                vp[k] = load4(p + i);
                vg[k] = load4(g + i);
                vm[k] = load4(m + i);
                vv[k] = load4(v + i);
            }
#pragma unroll
            for (int k = 0; k < kGroupsPerThread; ++k) {
                const int i = (k * 256 + (int)threadIdx.x) * 4;
                adamw_group(vp[k], vg[k], vm[k], vv[k], sc, step_size, bc2_sqrt);
                store4(p + i, vp[k]);
                store4(m + i, vm[k]);
                store4(v + i, vv[k]);
            }
        } else {                               // the entry's last chunk: whole groups as above, the last one by scalars
            for (int k = 0; k < kGroupsPerThread; ++k) {
                const int i = (k * 256 + (int)threadIdx.x) * 4;
                if (i + 4 <= len) {
                    opt_f4 vp = load4(p + i), vm = load4(m + i), vv = load4(v + i);
                    const opt_f4 vg = load4(g + i);
                    adamw_group(vp, vg, vm, vv, sc, step_size, bc2_sqrt);
                    store4(p + i, vp);
                    store4(m + i, vm);
                    store4(v + i, vv);
                } else {
                    for (int j = i; j < len; ++j) {
                        float ep = p[j], em = m[j], ev = v[j];
                        adamw_elem(ep, g[j], em, ev, sc, step_size, bc2_sqrt);
                        p[j] = ep; m[j] = em; v[j] = ev;
                    }
                }
            }
        }
    } else {                                   // any float address: one element per lane and round, coalesced dword accesses
        for (int j = (int)threadIdx.x; j < len; j += 256) {
            float ep = p[j], em = m[j], ev = v[j];
            adamw_elem(ep, g[j], em, ev, sc, step_size, bc2_sqrt);
            p[j] = ep; m[j] = em; v[j] = ev;
        }
    }
}

// One block: one chunk of one entry -> one fp64 partial (the chunk's sum of squares).
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const GradTable tab, int n, double* partials) {
    __shared__ double red[256];
    const int blk = blockIdx.x;
    const int ent = find_entry(tab, n, blk);
    const long long start = (long long)(blk - tab.e[ent].first_block) * kOptimChunk;
    const long long left = tab.e[ent].n - start;
    const int len = left < (long long)kOptimChunk ? (int)left : kOptimChunk;
    const float* g = tab.e[ent].g + start;
    double acc = 0.0;
    if (len == kOptimChunk) {
        opt_f4 vg[kGroupsPerThread];
#pragma unroll
        for (int k = 0; k < kGroupsPerThread; ++k) vg[k] = load4_any(g + (k * 256 + (int)threadIdx.x) * 4);
#pragma unroll
        for (int k = 0; k < kGroupsPerThread; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += (double)vg[k][j] * (double)vg[k][j];
    } else {
        for (int k = 0; k < kGroupsPerThread; ++k) {
            const int i = (k * 256 + (int)threadIdx.x) * 4;
            if (i + 4 <= len) {
                const opt_f4 vg = load4_any(g + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc += (double)vg[j] * (double)vg[j];
            } else {
                for (int j = i; j < len; ++j) acc += (double)g[j] * (double)g[j];
            }
        }
    }
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) partials[blk] = acc;
}

// One block: every partial of the list, ascending per thread, then the tree; total_norm = (float)sqrt(sum).
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* partials, long long n_partials, float* total_norm) {
    __shared__ double red[256];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) total_norm[0] = (float)sqrt(acc);
}

__global__ __launch_bounds__(256) void grad_clip_kernel(const GradTable tab, int n, const float* total_norm, float max_norm) {
    const float c = __fdiv_rn(max_norm, __fadd_rn(total_norm[0], 1e-6f));
    const float coef = c > 1.0f ? 1.0f : c;                    // NaN stays NaN, as torch.clamp(max=1.0) leaves it
    if (coef == 1.0f) return;                                  // x * 1.0f is x: nothing to load or store (false for NaN)
    const int blk = blockIdx.x;
    const int ent = find_entry(tab, n, blk);
    const long long start = (long long)(blk - tab.e[ent].first_block) * kOptimChunk;
    const long long left = tab.e[ent].n - start;
    const int len = left < (long long)kOptimChunk ? (int)left : kOptimChunk;
    float* g = tab.e[ent].g + start;
    if (aligned16(tab.e[ent].g)) {
        for (int k = 0; k < kGroupsPerThread; ++k) {
            const int i = (k * 256 + (int)threadIdx.x) * 4;
            if (i + 4 <= len) {
                opt_f4 vg = load4(g + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) vg[j] = __fmul_rn(vg[j], coef);
                store4(g + i, vg);
            } else {
                for (int j = i; j < len; ++j) g[j] = __fmul_rn(g[j], coef);
            }
        }
    } else {
        for (int j = (int)threadIdx.x; j < len; j += 256) g[j] = __fmul_rn(g[j], coef);
    }
}

static bool bad_group(int n, int blocks) { return n < 1 || n > kOptimMaxTensors || blocks < n; }

hipError_t launch_adamw_step(const AdamwTable& tab, int n, int blocks, const AdamwScalars& sc, hipStream_t s) {
    if (bad_group(n, blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(adamw_step_kernel, dim3(blocks), dim3(256), 0, s, tab, n, sc);
    return hipGetLastError();
}

hipError_t launch_grad_sumsq(const GradTable& tab, int n, int blocks, double* partials, hipStream_t s) {
    if (bad_group(n, blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, s, tab, n, partials);
    return hipGetLastError();
}

hipError_t launch_grad_norm_finish(const double* partials, long long n_partials, float* total_norm, hipStream_t s) {
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, s, partials, n_partials, total_norm);
    return hipGetLastError();
}

hipError_t launch_grad_clip(const GradTable& tab, int n, int blocks, const float* total_norm, float max_norm, hipStream_t s) {
    if (bad_group(n, blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grad_clip_kernel, dim3(blocks), dim3(256), 0, s, tab, n, total_norm, max_norm);
    return hipGetLastError();
}

}  // namespace st
