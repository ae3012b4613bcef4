// Training kernels of the MelStyleEncoder and the DurationPredictor (models/reference_encoder.py:22-93,
// models/duration_predictor.py:5-37): the row work of the training forward (activations kept, dropout applied) and the backward.
// fp32 throughout, as the inference forward (style_dp_kernels.hip); the data gradients of the convs are that file's tile kernel
// (launch_sd_conv_dgrad), the weight gradients fp32_tile.h's split-K TN GEMM on the fp32 MFMA.  No atomics anywhere: every reduction
// has a fixed order, so gradients are bitwise reproducible from run to run.
#include "fp32_tile.h"
#include "style_dp_drop.h"
#include "train_launch.h"

#include <math.h>

namespace st {

SdDrop sd_make_drop(float p, unsigned long long seed, int salt) {
    const DropCfg c = make_drop(p, seed, salt);
    SdDrop d;
    d.seed = c.seed; d.thresh16 = c.thresh16; d.scale = c.scale;
    return d;
}

// ---- weight gradient: dW[co][n] = sum_f dY[f][co] X'[f][n], n = ci * taps + j, f = (b, t) -----------------------------------
// fp32_tile.h's split-K kernel on the frames (b, t) of (B, C, T) tensors; X' = (in + addv) * imask, zero outside [0, T).
template <int TAPS>
struct SdWgradSrc {
    SdWgradArgs a;
    struct Frame { int b, t; };
    __host__ __device__ int cout() const { return a.Cout; }
    __host__ __device__ int n() const { return a.Cin * TAPS; }
    __host__ __device__ int64_t frames() const { return (int64_t)a.B * a.T; }
    __device__ Frame frame(int64_t f) const { const int b = (int)(f / a.T); return {b, (int)(f - (int64_t)b * a.T)}; }
    __device__ float dy(Frame f, int co) const { return a.dy[((size_t)f.b * a.Cout + co) * a.T + f.t]; }
    __device__ float x(Frame f, int nn) const {
        const int ci = nn / TAPS, tt = f.t + (nn - ci * TAPS) - TAPS / 2;
        if (tt < 0 || tt >= a.T) return 0.0f;
        float xv = a.in[((size_t)f.b * a.Cin + ci) * a.T + tt];
        if (a.addv) xv += a.addv[(size_t)f.b * a.Cin + ci];
        if (a.imask) xv *= a.imask[(size_t)f.b * a.T + tt];
        return xv;
    }
};

size_t sd_wgrad_scratch_floats(int B, int Cin, int Cout, int T, int taps) { return wgrad_scratch_floats((int64_t)B * T, Cout, Cin * taps); }

hipError_t launch_sd_wgrad(const SdWgradArgs& a, hipStream_t st) {
    if (a.B < 1 || a.T < 1 || a.Cin < 1 || a.Cout < 1 || !a.dy || !a.in || !a.dw) return hipErrorInvalidValue;
    switch (a.taps) {
        case 1: return launch_wgrad(SdWgradSrc<1>{a}, a.dw, a.scratch, st);
        case 3: return launch_wgrad(SdWgradSrc<3>{a}, a.dw, a.scratch, st);
        case 5: return launch_wgrad(SdWgradSrc<5>{a}, a.dw, a.scratch, st);
        default: return hipErrorInvalidValue;
    }
}

// ---- reductions over frames ----------------------------------------------------------------------------------------------
// One block per output (channel, or (item, channel)); 256 lanes stride the frames, a fixed LDS tree adds the partial sums.
__global__ __launch_bounds__(256) void sd_sum_frames_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, int T, int per_item) {
    __shared__ float red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int b0 = per_item ? blockIdx.y : 0, b1 = per_item ? blockIdx.y + 1 : B;
    float v = 0.0f;
    for (int b = b0; b < b1; ++b) {
        const float* xr = x + ((size_t)b * C + c) * T;
        for (int t = tid; t < T; t += 256) v += xr[t];
    }
    const float sum = block_sum256(red, v);
    if (tid == 0) out[per_item ? (size_t)blockIdx.y * C + c : (size_t)c] = sum;
}

hipError_t launch_sd_sum_frames(const float* x, float* out, int B, int C, int T, int per_item, hipStream_t s) {
    hipLaunchKernelGGL(sd_sum_frames_kernel, dim3(C, per_item ? B : 1), dim3(256), 0, s, x, out, B, C, T, per_item);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void sd_mul_mask_kernel(const float* __restrict__ x, const float* __restrict__ mask, float* __restrict__ y,
                                                          int C, int T, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / ((int64_t)C * T), t = i % T;
        y[i] = x[i] * mask[b * T + t];
    }
}

hipError_t launch_sd_mul_mask(const float* x, const float* mask, float* y, int B, int C, int T, hipStream_t s) {
    const int64_t n = (int64_t)B * C * T;
    hipLaunchKernelGGL(sd_mul_mask_kernel, dim3(grid_1d(n, 4096)), dim3(256), 0, s, x, mask, y, C, T, n);
    return hipGetLastError();
}

// ---- Mish (the forward is sd_conv_kernel's epilogue, launch_sd_conv_pre keeps the pre-activation) ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sd_drop_kernel(float* __restrict__ x, SdDrop d, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        x[i] *= sd_drop_elem(d, (unsigned long long)i);
}

__global__ __launch_bounds__(256) void sd_mish_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ pre, float* __restrict__ dpre,
                                                          SdDrop d, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float x = pre[i];
        const float sp = x > 20.0f ? x : log1pf(expf(x));
        const float tsp = tanhf(sp), sig = 1.0f / (1.0f + expf(-x));
        dpre[i] = dout[i] * sd_drop_elem(d, (unsigned long long)i) * (tsp + x * sig * (1.0f - tsp * tsp));
    }
}

hipError_t launch_sd_drop(float* x, const SdDrop& d, int64_t n, hipStream_t s) {
    if (!d.thresh16) return hipSuccess;      // p = 0: factor 1 everywhere
    hipLaunchKernelGGL(sd_drop_kernel, dim3(grid_1d(n, 4096)), dim3(256), 0, s, x, d, n);
    return hipGetLastError();
}

hipError_t launch_sd_mish_bwd(const float* dout, const float* pre, float* dpre, const SdDrop& d, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(sd_mish_bwd_kernel, dim3(grid_1d(n, 4096)), dim3(256), 0, s, dout, pre, dpre, d, n);
    return hipGetLastError();
}

// ---- Conv1dGLU tail ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sd_glu_train_kernel(const float* __restrict__ hin, const float* __restrict__ u, float* __restrict__ hout,
                                                           SdDrop d, int C, int T, int64_t n) {
    const int64_t per = (int64_t)C * T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / per, rem = i - b * per;
        const float* ub = u + b * 2 * per;
        const float val = ub[rem], gate = ub[per + rem];
        const float sig = 1.0f / (1.0f + expf(-gate));
        // p = 0: one fma, as sd_glu_residual_kernel's h + val * sig compiles (bitwise the inference value)
        hout[i] = d.thresh16 ? fmaf(val * sig, sd_drop_elem(d, (unsigned long long)i), hin[i]) : fmaf(val, sig, hin[i]);
    }
}

__global__ __launch_bounds__(256) void sd_glu_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ u, float* __restrict__ du,
                                                         SdDrop d, int C, int T, int64_t n) {
    const int64_t per = (int64_t)C * T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / per, rem = i - b * per;
        const float* ub = u + b * 2 * per;
        float* db = du + b * 2 * per;
        const float val = ub[rem], sig = 1.0f / (1.0f + expf(-ub[per + rem]));
        const float g = dh[i] * sd_drop_elem(d, (unsigned long long)i);
        db[rem] = g * sig;
        db[per + rem] = g * val * sig * (1.0f - sig);
    }
}

hipError_t launch_sd_glu_train(const float* hin, const float* u, float* hout, const SdDrop& d, int B, int C, int T, hipStream_t s) {
    const int64_t n = (int64_t)B * C * T;
    hipLaunchKernelGGL(sd_glu_train_kernel, dim3(grid_1d(n, 4096)), dim3(256), 0, s, hin, u, hout, d, C, T, n);
    return hipGetLastError();
}

hipError_t launch_sd_glu_bwd(const float* dh, const float* u, float* du, const SdDrop& d, int B, int C, int T, hipStream_t s) {
    const int64_t n = (int64_t)B * C * T;
    hipLaunchKernelGGL(sd_glu_bwd_kernel, dim3(grid_1d(n, 4096)), dim3(256), 0, s, dh, u, du, d, C, T, n);
    return hipGetLastError();
}

// ---- channel LayerNorm ---------------------------------------------------------------------------------------------------
// Forward: sd_layernorm_channels_kernel's arithmetic (same reduction order: bitwise the inference values before dropout),
// out of place, with the statistics kept.  One block = 64 frames of one item, 4 threads per frame split the channels.
__global__ __launch_bounds__(256) void sd_layernorm_train_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ mean_out,
                                                                 float* __restrict__ rstd_out, const float* __restrict__ w, const float* __restrict__ bb,
                                                                 float eps, SdDrop d, int C, int T) {
    __shared__ float red[4][64];
    const int tl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + tl, b = blockIdx.y;
    const bool ok = t < T;
    const float* xb = x + (size_t)b * C * T;
    float* yb = y + (size_t)b * C * T;
    float sum = 0.0f;
    if (ok) for (int c = g; c < C; c += 4) sum += xb[(size_t)c * T + t];
    red[g][tl] = sum;
    __syncthreads();
    const float mean = (red[0][tl] + red[1][tl] + red[2][tl] + red[3][tl]) / (float)C;
    __syncthreads();
    float sq = 0.0f;
    if (ok) for (int c = g; c < C; c += 4) { const float dv = xb[(size_t)c * T + t] - mean; sq += dv * dv; }
    red[g][tl] = sq;
    __syncthreads();
    const float var = (red[0][tl] + red[1][tl] + red[2][tl] + red[3][tl]) / (float)C;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (!ok) return;
    if (g == 0) { mean_out[(size_t)b * T + t] = mean; rstd_out[(size_t)b * T + t] = rstd; }
    for (int c = g; c < C; c += 4) {
        const size_t i = (size_t)c * T + t;
        const float v = (xb[i] - mean) * rstd * w[c] + bb[c];
        yb[i] = v * sd_drop_elem(d, (unsigned long long)((size_t)b * C * T + i));
    }
}

hipError_t launch_sd_layernorm_train(const float* x, float* y, float* mean, float* rstd, const float* w, const float* b, float eps,
                                     const SdDrop& d, int B, int C, int T, hipStream_t s) {
    hipLaunchKernelGGL(sd_layernorm_train_kernel, dim3((T + 63) / 64, B), dim3(256), 0, s, x, y, mean, rstd, w, b, eps, d, C, T);
    return hipGetLastError();
}

// dx per frame (same block shape as the forward)
__global__ __launch_bounds__(256) void sd_layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean_in,
                                                               const float* __restrict__ rstd_in, const float* __restrict__ w, float* __restrict__ dx,
                                                               SdDrop d, int relu_x, int C, int T) {
    __shared__ float red[2][4][64];
    const int tl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + tl, b = blockIdx.y;
    const bool ok = t < T;
    const size_t base = (size_t)b * C * T;
    const float mean = ok ? mean_in[(size_t)b * T + t] : 0.0f, rstd = ok ? rstd_in[(size_t)b * T + t] : 0.0f;
    float s1 = 0.0f, s2 = 0.0f;
    if (ok) for (int c = g; c < C; c += 4) {
        const size_t i = base + (size_t)c * T + t;
        const float gw = dy[i] * sd_drop_elem(d, (unsigned long long)i) * w[c];
        s1 += gw;
        s2 += gw * ((x[i] - mean) * rstd);
    }
    red[0][g][tl] = s1; red[1][g][tl] = s2;
    __syncthreads();
    const float m1 = (red[0][0][tl] + red[0][1][tl] + red[0][2][tl] + red[0][3][tl]) / (float)C;
    const float m2 = (red[1][0][tl] + red[1][1][tl] + red[1][2][tl] + red[1][3][tl]) / (float)C;
    if (!ok) return;
    for (int c = g; c < C; c += 4) {
        const size_t i = base + (size_t)c * T + t;
        const float xv = x[i];
        const float gw = dy[i] * sd_drop_elem(d, (unsigned long long)i) * w[c];
        float v = rstd * (gw - m1 - (xv - mean) * rstd * m2);
        if (relu_x && !(xv > 0.0f)) v = 0.0f;
        dx[i] = v;
    }
}

// dw / db: one block per channel, the (item, frame) pairs in a fixed order
__global__ __launch_bounds__(256) void sd_layernorm_param_grad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                      const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                                      float* __restrict__ dw, float* __restrict__ db, SdDrop d, int B, int C, int T) {
    __shared__ float r1[256], r2[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    float sw = 0.0f, sb = 0.0f;
    for (int b = 0; b < B; ++b) {
        for (int t = tid; t < T; t += 256) {
            const size_t i = ((size_t)b * C + c) * T + t;
            const float dn = dy[i] * sd_drop_elem(d, (unsigned long long)i);
            sb += dn;
            sw += dn * ((x[i] - mean_in[(size_t)b * T + t]) * rstd_in[(size_t)b * T + t]);
        }
    }
    r1[tid] = sw; r2[tid] = sb;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { r1[tid] += r1[tid + w]; r2[tid] += r2[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) { dw[c] = r1[0]; db[c] = r2[0]; }
}

hipError_t launch_sd_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* w, float* dx,
                                   float* dw, float* db, const SdDrop& d, int relu_x, int B, int C, int T, hipStream_t s) {
    hipLaunchKernelGGL(sd_layernorm_bwd_kernel, dim3((T + 63) / 64, B), dim3(256), 0, s, dy, x, mean, rstd, w, dx, d, relu_x, C, T);
    hipLaunchKernelGGL(sd_layernorm_param_grad_kernel, dim3(C), dim3(256), 0, s, dy, x, mean, rstd, dw, db, d, B, C, T);
    return hipGetLastError();
}

// ---- attention backward (head_dim 64) ------------------------------------------------------------------------------------
// P[q][k] = exp(s - m_q) / l_q recomputed from the forward's statistics, s = (q / 8) . k as the forward's fma order; the
// dropped probabilities P o Z (Z = keep / (1 - p)) produced O.  With D_q = dO_q . O_q:
//   dV = (P o Z)^T dO,  dS = P o (Z o (dO V^T) - D),  dQ = dS K / 8,  dK = dS^T (Q / 8).
// Pass 1: one lane per query (dq, D).  Pass 2: one lane per key (dk, dv); both stream the other side through LDS.
__global__ __launch_bounds__(64) void sd_attention_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ kmask,
                                                                const float* __restrict__ out, const float* __restrict__ dout,
                                                                const float* __restrict__ stats, float* __restrict__ dsum,
                                                                float* __restrict__ dqkv, SdDrop drop, int H, int T) {
    __shared__ float Ks[64 * 64];
    __shared__ float Vs[64 * 64];
    __shared__ float valid[64];
    const int lane = threadIdx.x, hd = blockIdx.y, b = blockIdx.z, B = gridDim.z;
    const int tq = blockIdx.x * 64 + lane, D = H * 64;
    const bool qok = tq < T;
    const float* qb = qkv + ((size_t)b * 3 * D + hd * 64) * T;
    const float* kb = qb + (size_t)D * T;
    const float* vb = qb + (size_t)2 * D * T;
    const float* ob = out + ((size_t)b * D + hd * 64) * T;
    const float* gb = dout + ((size_t)b * D + hd * 64) * T;
    const size_t row = (size_t)(b * H + hd) * T + tq;
    float q[64], go[64], dq[64];
    float Dq = 0.0f;
#pragma unroll
    for (int e = 0; e < 64; ++e) {
        q[e] = qok ? qb[(size_t)e * T + tq] * 0.125f : 0.0f;
        go[e] = qok ? gb[(size_t)e * T + tq] : 0.0f;
        Dq = fmaf(go[e], qok ? ob[(size_t)e * T + tq] : 0.0f, Dq);
        dq[e] = 0.0f;
    }
    const float m = qok ? stats[row] : 0.0f, il = qok ? stats[(size_t)B * H * T + row] : 0.0f;
    if (qok) dsum[row] = Dq;
    for (int k0 = 0; k0 < T; k0 += 64) {
        const int tk = k0 + lane;
        const bool kv = tk < T && (!kmask || kmask[(size_t)b * T + tk] != 0.0f);
        for (int e = 0; e < 64; ++e) {
            Ks[e * 64 + lane] = tk < T ? kb[(size_t)e * T + tk] : 0.0f;
            Vs[e * 64 + lane] = tk < T ? vb[(size_t)e * T + tk] : 0.0f;
        }
        valid[lane] = kv ? 1.0f : 0.0f;
        __syncthreads();
        if (il != 0.0f) {
            for (int j = 0; j < 64; ++j) {
                if (valid[j] == 0.0f) continue;
                float s = 0.0f, dp = 0.0f;
#pragma unroll
                for (int e = 0; e < 64; ++e) { s = fmaf(q[e], Ks[e * 64 + j], s); dp = fmaf(go[e], Vs[e * 64 + j], dp); }
                const float p = expf(s - m) * il;
                const float ds = p * (dp * sd_drop_attn(drop, (unsigned)row, (unsigned)(k0 + j)) - Dq);
#pragma unroll
                for (int e = 0; e < 64; ++e) dq[e] = fmaf(ds, Ks[e * 64 + j], dq[e]);
            }
        }
        __syncthreads();
    }
    if (!qok) return;
    float* db = dqkv + ((size_t)b * 3 * D + hd * 64) * T + tq;
#pragma unroll
    for (int e = 0; e < 64; ++e) db[(size_t)e * T] = dq[e] * 0.125f;
}

__global__ __launch_bounds__(64) void sd_attention_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ kmask,
                                                                 const float* __restrict__ dout, const float* __restrict__ stats,
                                                                 const float* __restrict__ dsum, float* __restrict__ dqkv, SdDrop drop, int H, int T) {
    __shared__ float Qs[64 * 64];
    __shared__ float Gs[64 * 64];
    __shared__ float Ms[64], Ls[64], Ds[64];
    const int lane = threadIdx.x, hd = blockIdx.y, b = blockIdx.z, B = gridDim.z;
    const int tk = blockIdx.x * 64 + lane, D = H * 64;
    const bool kok = tk < T && (!kmask || kmask[(size_t)b * T + tk] != 0.0f);
    const float* qb = qkv + ((size_t)b * 3 * D + hd * 64) * T;
    const float* kb = qb + (size_t)D * T;
    const float* vb = qb + (size_t)2 * D * T;
    const float* gb = dout + ((size_t)b * D + hd * 64) * T;
    const size_t row0 = (size_t)(b * H + hd) * T;
    float k[64], v[64], dk[64], dv[64];
#pragma unroll
    for (int e = 0; e < 64; ++e) {
        k[e] = kok ? kb[(size_t)e * T + tk] : 0.0f;
        v[e] = kok ? vb[(size_t)e * T + tk] : 0.0f;
        dk[e] = 0.0f; dv[e] = 0.0f;
    }
    for (int q0 = 0; q0 < T; q0 += 64) {
        const int tq = q0 + lane;
        const bool qok = tq < T;
        for (int e = 0; e < 64; ++e) {
            Qs[e * 64 + lane] = qok ? qb[(size_t)e * T + tq] * 0.125f : 0.0f;
            Gs[e * 64 + lane] = qok ? gb[(size_t)e * T + tq] : 0.0f;
        }
        Ms[lane] = qok ? stats[row0 + tq] : 0.0f;
        Ls[lane] = qok ? stats[(size_t)B * H * T + row0 + tq] : 0.0f;
        Ds[lane] = qok ? dsum[row0 + tq] : 0.0f;
        __syncthreads();
        if (kok) {
            for (int i = 0; i < 64; ++i) {
                const float il = Ls[i];
                if (il == 0.0f) continue;
                float s = 0.0f, dp = 0.0f;
#pragma unroll
                for (int e = 0; e < 64; ++e) { s = fmaf(Qs[e * 64 + i], k[e], s); dp = fmaf(Gs[e * 64 + i], v[e], dp); }
                const float p = expf(s - Ms[i]) * il;
                const float z = sd_drop_attn(drop, (unsigned)(row0 + q0 + i), (unsigned)tk);
                const float pz = p * z, ds = p * (dp * z - Ds[i]);
#pragma unroll
                for (int e = 0; e < 64; ++e) { dv[e] = fmaf(pz, Gs[e * 64 + i], dv[e]); dk[e] = fmaf(ds, Qs[e * 64 + i], dk[e]); }
            }
        }
        __syncthreads();
    }
    if (tk >= T) return;
    float* dkb = dqkv + ((size_t)b * 3 * D + D + hd * 64) * T + tk;
    float* dvb = dkb + (size_t)D * T;
#pragma unroll
    for (int e = 0; e < 64; ++e) { dkb[(size_t)e * T] = dk[e]; dvb[(size_t)e * T] = dv[e]; }
}

hipError_t launch_sd_attention_bwd(const float* qkv, const float* kmask, const float* out, const float* dout, const float* stats,
                                   float* dsum, float* dqkv, const SdDrop& d, int B, int H, int T, hipStream_t s) {
    const dim3 grid((T + 63) / 64, H, B);
    hipLaunchKernelGGL(sd_attention_bwd_q_kernel, grid, dim3(64), 0, s, qkv, kmask, out, dout, stats, dsum, dqkv, d, H, T);
    hipLaunchKernelGGL(sd_attention_bwd_kv_kernel, grid, dim3(64), 0, s, qkv, kmask, dout, stats, dsum, dqkv, d, H, T);
    return hipGetLastError();
}

// ---- masked mean-pool backward -------------------------------------------------------------------------------------------
// One block per (channel, item): the valid-frame count as sd_mean_pool_kernel counts it, then dc / n on the valid frames.
__global__ __launch_bounds__(256) void sd_mean_pool_bwd_kernel(const float* __restrict__ dc, const float* __restrict__ mask, float* __restrict__ dx,
                                                               int O, int T) {
    __shared__ float scnt[256];
    const int o = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* mb = mask ? mask + (size_t)b * T : nullptr;
    float n = 0.0f;
    for (int t = tid; t < T; t += 256) if (!mb || mb[t] != 0.0f) n += 1.0f;
    const float cnt = block_sum256(scnt, n);
    const float g = cnt > 0.0f ? dc[(size_t)b * O + o] / cnt : 0.0f;
    float* xo = dx + ((size_t)b * O + o) * T;
    for (int t = tid; t < T; t += 256) xo[t] = (!mb || mb[t] != 0.0f) ? g : 0.0f;
}

hipError_t launch_sd_mean_pool_bwd(const float* dc, const float* mask, float* dx, int B, int O, int T, hipStream_t s) {
    hipLaunchKernelGGL(sd_mean_pool_bwd_kernel, dim3(O, B), dim3(256), 0, s, dc, mask, dx, O, T);
    return hipGetLastError();
}

}  // namespace st
