// Training side of the alignment step of StableTTS.forward (models/model.py:160-176) and duration_loss
// (models/duration_predictor.py:38-40): gather, masking, prior loss, duration loss and their gradients, from the per-token
// frame counts the alignment search wrote.  HBM-bound, small work: plain loads and stores, time contiguous in every tensor.
// Sums that decide a gradient or a loss accumulate in fp64 in one fixed order (per thread ascending, then a fixed tree):
// no atomics, nothing depends on the grid, the batch or the neighbouring tokens.
#include "common.h"
#include "block_reduce.h"
#include "align_train_launch.h"

namespace st {

namespace {

constexpr float kLog2Pi = 1.8378770664093453f;

// frames of token j as the kernels count them: only where x_mask != 0, a negative count is 0, never more than Ty
__device__ __forceinline__ long long clipped_count(const int32_t* dur, const float* xm, int j, int Ty) {
    int d = dur[j];
    d = d < 0 ? 0 : (d > Ty ? Ty : d);
    return xm[j] != 0.f ? (long long)d : 0ll;
}

// ends[i] = min(sum_{j <= i} count_j, Ty) for one item (dur, xm: its rows), i < Tx <= kAlignTrainMaxTx: token i owns the
// frames [ends[i-1], ends[i]).  The clip happens here, before anything is indexed.  256 threads; part: 256 int64 of LDS.
__device__ __forceinline__ void segment_ends(const int32_t* dur, const float* xm, int Tx, int Ty, int* ends, long long* part) {
    const int tid = threadIdx.x;
    const int chunk = (Tx + 255) / 256;
    const int lo = tid * chunk < Tx ? tid * chunk : Tx;
    const int hi = lo + chunk < Tx ? lo + chunk : Tx;
    long long s = 0;
    for (int j = lo; j < hi; ++j) s += clipped_count(dur, xm, j, Ty);
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {          // inclusive scan of the 256 chunk sums
        const long long v = tid >= off ? part[tid - off] : 0ll;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long long run = tid ? part[tid - 1] : 0ll;
    for (int j = lo; j < hi; ++j) {
        run += clipped_count(dur, xm, j, Ty);
        ends[j] = (int)(run < (long long)Ty ? run : (long long)Ty);
    }
    __syncthreads();
}

}  // namespace

// one block: 256 consecutive frames x kAlignTrainChannels channels of one item
__global__ __launch_bounds__(256) void align_train_fwd_kernel(const int32_t* durations, const float* x_mask, const float* y_mask,
                                                              const float* mu_x, const float* y, const float* fake_content,
                                                              const float* keep, int M, int Tx, int Ty, int nblk,
                                                              int32_t* frame_token, float* mu_y, float* mu_y_masked, float* scratch) {
    __shared__ int ends[kAlignTrainMaxTx];
    __shared__ long long part[256];
    __shared__ float red[2][4];
    const int b = blockIdx.z;
    segment_ends(durations + (size_t)b * Tx, x_mask + (size_t)b * Tx, Tx, Ty, ends, part);
    const int t = blockIdx.x * kAlignTrainFrames + threadIdx.x;
    float acc = 0.f, am = 0.f;
    if (t < Ty) {
        int lo = 0, hi = Tx;                    // first token whose range ends after t: it has frames, so x_mask != 0 there
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (t < ends[mid]) hi = mid; else lo = mid + 1; }
        const int tok = lo < Tx ? lo : -1;
        const float ym = y_mask[(size_t)b * Ty + t];
        if (blockIdx.y == 0) { frame_token[(size_t)b * Ty + t] = tok; am = ym; }
        const float k = (keep && keep[b] == 0.f) ? 0.f : 1.f;
        const int m0 = blockIdx.y * kAlignTrainChannels;
        const int m1 = m0 + kAlignTrainChannels < M ? m0 + kAlignTrainChannels : M;
        for (int m = m0; m < m1; ++m) {
            const float v = tok >= 0 ? mu_x[((size_t)b * M + m) * Tx + tok] : 0.f;
            const size_t o = ((size_t)b * M + m) * Ty + t;
            if (mu_y) mu_y[o] = v;
            const float fc = fake_content ? fake_content[m] : 0.f;
            mu_y_masked[o] = v * k + (1.f - k) * fc;          // mu_y * cfg_mask + ~cfg_mask * fake_content (model.py:172)
            const float d = y[o] - v;
            acc += 0.5f * (d * d + kLog2Pi) * ym;             // model.py:175
        }
    }
    acc = wave_sum(acc); am = wave_sum(am);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = acc; red[1][threadIdx.x >> 6] = am; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        scratch[blk] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        scratch[nblk + blk] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

__global__ __launch_bounds__(256) void align_train_prior_final_kernel(float* scratch, int nblk, int M, float* prior_loss) {
    __shared__ double red[256];
    double a = 0.0, m = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) { a += (double)scratch[i]; m += (double)scratch[nblk + i]; }
    a = block_sum_f64(a, red);
    m = block_sum_f64(m, red);
    if (threadIdx.x == 0) {
        const float den = (float)m * (float)M;                // torch.sum(y_mask) * mel_channels, fp32 (model.py:176)
        scratch[2 * nblk] = (float)a; scratch[2 * nblk + 1] = den;
        *prior_loss = (float)(a / (double)den);
    }
}

int align_train_scratch_floats(int B, int M, int Ty) {
    const long long gx = (Ty + kAlignTrainFrames - 1) / kAlignTrainFrames, gy = (M + kAlignTrainChannels - 1) / kAlignTrainChannels;
    const long long n = 2 * gx * gy * (long long)B + 2;
    return n > 0x7fffffffll ? -1 : (int)n;
}

hipError_t launch_align_train_forward(const int32_t* durations, const float* x_mask, const float* y_mask, const float* mu_x,
                                      const float* y, const float* fake_content, const float* keep, int B, int M, int Tx, int Ty,
                                      int32_t* frame_token, float* mu_y, float* mu_y_masked, float* scratch, float* prior_loss,
                                      hipStream_t s) {
    if (Tx > kAlignTrainMaxTx || align_train_scratch_floats(B, M, Ty) < 0) return hipErrorInvalidValue;
    const dim3 grid((Ty + kAlignTrainFrames - 1) / kAlignTrainFrames, (M + kAlignTrainChannels - 1) / kAlignTrainChannels, B);
    const int nblk = (int)(grid.x * grid.y * grid.z);
    hipLaunchKernelGGL(align_train_fwd_kernel, grid, dim3(256), 0, s, durations, x_mask, y_mask, mu_x, y, fake_content, keep, M, Tx,
                       Ty, nblk, frame_token, mu_y, mu_y_masked, scratch);
    hipLaunchKernelGGL(align_train_prior_final_kernel, dim3(1), dim3(256), 0, s, scratch, nblk, M, prior_loss);
    return hipGetLastError();
}

// one block: 64 consecutive tokens (the lanes of a wave) x kAlignTrainChannels channels (4 per wave) of one item.  A thread
// walks the frames of its own token in ascending order, however many they are; consecutive lanes own consecutive frame
// ranges, so the wave's loads stay close together.
__global__ __launch_bounds__(256) void align_train_bwd_kernel(const int32_t* durations, const float* x_mask, const float* y_mask,
                                                              const float* mu_x, const float* y, const float* keep,
                                                              const float* scratch, int den_at, const float* g_masked,
                                                              const float* g_mu_y, const float* g_prior, int M, int Tx, int Ty,
                                                              float* grad_mu_x) {
    __shared__ int ends[kAlignTrainMaxTx];
    __shared__ long long part[256];
    const int b = blockIdx.z;
    segment_ends(durations + (size_t)b * Tx, x_mask + (size_t)b * Tx, Tx, Ty, ends, part);
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    if (i >= Tx) return;
    const int t0 = i > 0 ? ends[i - 1] : 0, t1 = ends[i];     // 0 <= t0 <= t1 <= Ty
    const double k = (keep && keep[b] == 0.f) ? 0.0 : 1.0;
    const double c = g_prior ? (double)g_prior[0] / (double)scratch[den_at] : 0.0;
    const float* ym = y_mask + (size_t)b * Ty;
    const int m0 = blockIdx.y * kAlignTrainChannels + (threadIdx.x >> 6);
    const int m1 = (blockIdx.y + 1) * kAlignTrainChannels < M ? (blockIdx.y + 1) * kAlignTrainChannels : M;
    for (int m = m0; m < m1; m += 4) {
        const size_t row = ((size_t)b * M + m) * Ty;
        const double mu = (double)mu_x[((size_t)b * M + m) * Tx + i];
        double acc = 0.0;
        for (int t = t0; t < t1; ++t) {
            double term = 0.0;
            if (g_masked) term = k * (double)g_masked[row + t];
            if (g_mu_y) term += (double)g_mu_y[row + t];
            if (g_prior) term += c * (double)ym[t] * (mu - (double)y[row + t]);
            acc += term;
        }
        grad_mu_x[((size_t)b * M + m) * Tx + i] = (float)acc;
    }
}

// grad_fake_content[m]: one block per channel; a thread sums its frames of every dropped item, ascending, then the fixed tree
__global__ __launch_bounds__(256) void align_train_fake_bwd_kernel(const float* keep, const float* g_masked, int B, int M, int Ty,
                                                                   float* grad_fake_content) {
    __shared__ double red[256];
    const int m = blockIdx.x;
    double acc = 0.0;
    if (keep && g_masked)
        for (int b = 0; b < B; ++b) {
            if (keep[b] != 0.f) continue;
            const float* g = g_masked + ((size_t)b * M + m) * Ty;
            for (int t = threadIdx.x; t < Ty; t += 256) acc += (double)g[t];
        }
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) grad_fake_content[m] = (float)acc;
}

hipError_t launch_align_train_backward(const int32_t* durations, const float* x_mask, const float* y_mask, const float* mu_x,
                                       const float* y, const float* keep, const float* scratch, const float* g_masked,
                                       const float* g_mu_y, const float* g_prior, int B, int M, int Tx, int Ty, float* grad_mu_x,
                                       float* grad_fake_content, hipStream_t s) {
    const int nfloats = align_train_scratch_floats(B, M, Ty);
    if (Tx > kAlignTrainMaxTx || nfloats < 0) return hipErrorInvalidValue;
    const dim3 grid((Tx + 63) / 64, (M + kAlignTrainChannels - 1) / kAlignTrainChannels, B);
    hipLaunchKernelGGL(align_train_bwd_kernel, grid, dim3(256), 0, s, durations, x_mask, y_mask, mu_x, y, keep, scratch, nfloats - 1,
                       g_masked, g_mu_y, g_prior, M, Tx, Ty, grad_mu_x);
    if (grad_fake_content)
        hipLaunchKernelGGL(align_train_fake_bwd_kernel, dim3(M), dim3(256), 0, s, keep, g_masked, B, M, Ty, grad_fake_content);
    return hipGetLastError();
}

// ---- duration loss.  d = logw - log(1e-8 + durations) * x_mask in fp64: where the prediction is close to its target the
// difference cancels, and an fp32 log would leave the gradient with the target's rounding error instead of its own.
__device__ __forceinline__ double dur_target(const int32_t* durations, const float* x_mask, int64_t i) {
    const int d = durations[i];
    return log(1e-8 + (double)(d < 0 ? 0 : d)) * (double)x_mask[i];
}

__global__ __launch_bounds__(256) void duration_loss_partial_kernel(const float* logw, const int32_t* durations, const float* x_mask,
                                                                    int64_t n, float* logw_target, float* scratch) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double tgt = dur_target(durations, x_mask, i);
        if (logw_target) logw_target[i] = (float)tgt;
        const double d = (double)logw[i] - tgt;
        acc += d * d;
    }
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) scratch[blockIdx.x] = (float)acc;
}

__global__ __launch_bounds__(256) void duration_loss_final_kernel(float* scratch, int nblocks, const long long* x_lengths, int B,
                                                                  float* loss) {
    __shared__ double red[256];
    double a = 0.0, len = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) a += (double)scratch[i];
    for (int i = threadIdx.x; i < B; i += 256) len += (double)x_lengths[i];
    a = block_sum_f64(a, red);
    len = block_sum_f64(len, red);
    if (threadIdx.x == 0) {
        const float den = (float)len;                          // torch.sum(lengths) promoted to fp32 (duration_predictor.py:39)
        scratch[kDurLossBlocks] = (float)a; scratch[kDurLossBlocks + 1] = den;
        *loss = (float)(a / (double)den);
    }
}

hipError_t launch_duration_loss(const float* logw, const int32_t* durations, const float* x_mask, const long long* x_lengths,
                                int B, int Tx, float* logw_target, float* scratch, float* loss, hipStream_t s) {
    const int64_t n = (int64_t)B * Tx;
    int grid = (int)((n + 255) / 256); if (grid > kDurLossBlocks) grid = kDurLossBlocks; if (grid < 1) grid = 1;
    hipLaunchKernelGGL(duration_loss_partial_kernel, dim3(grid), dim3(256), 0, s, logw, durations, x_mask, n, logw_target, scratch);
    hipLaunchKernelGGL(duration_loss_final_kernel, dim3(1), dim3(256), 0, s, scratch, grid, x_lengths, B, loss);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void duration_loss_bwd_kernel(const float* logw, const int32_t* durations, const float* x_mask,
                                                                const float* scratch, const float* grad_loss, int64_t n,
                                                                float* grad_logw) {
    const double f = 2.0 * (double)grad_loss[0] / (double)scratch[kDurLossBlocks + 1];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        grad_logw[i] = (float)(f * ((double)logw[i] - dur_target(durations, x_mask, i)));
}

hipError_t launch_duration_loss_bwd(const float* logw, const int32_t* durations, const float* x_mask, const float* scratch,
                                    const float* grad_loss, int B, int Tx, float* grad_logw, hipStream_t s) {
    const int64_t n = (int64_t)B * Tx;
    int grid = (int)((n + 255) / 256); if (grid > 1024) grid = 1024; if (grid < 1) grid = 1;
    hipLaunchKernelGGL(duration_loss_bwd_kernel, dim3(grid), dim3(256), 0, s, logw, durations, x_mask, scratch, grad_loss, n, grad_logw);
    return hipGetLastError();
}

}  // namespace st
