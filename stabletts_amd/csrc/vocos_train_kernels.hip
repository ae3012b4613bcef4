// Vocos training kernels (vocoders/vocos/models/backbone.py:50-56, module.py:33-46, head.py:39-72,93-117 under autograd):
// what the fp32 training forward and the backward need around the fp32 MFMA GEMMs of style_dp_kernels.hip / style_dp_bwd.hip.
// Tensors are fp32 and channel-major over the flattened frames of the batch, (C, R) with R = B * T and r = b * T + t, so that
// the lanes of a wave read consecutive frames.  The kernels that mix frames (embed im2col, depthwise conv, ISTFT) take T and
// stay inside an item.  No atomics: every reduction is a per-thread strided sum followed by a fixed LDS tree.
#include "fp32_tile.h"
#include "vocos_train_launch.h"

#include <math.h>

namespace st {

// ---------------------------------------------------------------- embed: im2col of the k = 7 conv and its transpose
__global__ __launch_bounds__(256) void vt_im2col7_kernel(const float* __restrict__ mel, float* __restrict__ cols, int M, int T, int64_t R, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / R, r = i - row * R;
        const int ci = (int)(row / 7), j = (int)(row - (int64_t)ci * 7);
        const int64_t b = r / T;
        const int t = (int)(r - b * T), tt = t + j - 3;
        cols[i] = (tt >= 0 && tt < T) ? mel[(b * M + ci) * T + tt] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void vt_col2im7_kernel(const float* __restrict__ dcols, float* __restrict__ dmel, int M, int T, int64_t R, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {      // i = (b * M + ci) * T + t
        const int t = (int)(i % T);
        const int64_t bc = i / T, b = bc / M;
        const int ci = (int)(bc - b * M);
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int tt = t - j + 3;
            if (tt >= 0 && tt < T) acc += dcols[((int64_t)ci * 7 + j) * R + b * T + tt];
        }
        dmel[i] = acc;
    }
}

hipError_t launch_vt_im2col7(const float* mel, float* cols, int B, int M, int T, hipStream_t s) {
    const int64_t R = (int64_t)B * T, n = 7 * (int64_t)M * R;
    hipLaunchKernelGGL(vt_im2col7_kernel, dim3(grid_1d(n, 8192)), dim3(256), 0, s, mel, cols, M, T, R, n);
    return hipGetLastError();
}

hipError_t launch_vt_col2im7(const float* dcols, float* dmel, int B, int M, int T, hipStream_t s) {
    const int64_t R = (int64_t)B * T, n = (int64_t)M * R;
    hipLaunchKernelGGL(vt_col2im7_kernel, dim3(grid_1d(n, 8192)), dim3(256), 0, s, dcols, dmel, M, T, R, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------- depthwise k = 7 conv (module.py:35) and its backward
__global__ __launch_bounds__(256) void vt_dwconv7_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         float* __restrict__ z, int T, int64_t R, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t c = i / R, r = i - c * R;
        const int t = (int)(r % T);
        float acc = bias[c];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int tt = t + j - 3;
            if (tt >= 0 && tt < T) acc = fmaf(w[c * 7 + j], x[i + j - 3], acc);
        }
        z[i] = acc;
    }
}

__global__ __launch_bounds__(256) void vt_dwconv7_dx_kernel(const float* __restrict__ dz, const float* __restrict__ w, const float* __restrict__ dres,
                                                            float* __restrict__ dx, int T, int64_t R, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t c = i / R, r = i - c * R;
        const int t = (int)(r % T);
        float acc = dres[i];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int tt = t - j + 3;
            if (tt >= 0 && tt < T) acc = fmaf(w[c * 7 + j], dz[i - j + 3], acc);
        }
        dx[i] = acc;
    }
}

// one block per channel: 7 tap sums and the bias sum, the frames strided over the lanes, then a fixed LDS tree
__global__ __launch_bounds__(256) void vt_dwconv7_param_kernel(const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ dw,
                                                               float* __restrict__ db, int T, int64_t R) {
    __shared__ float red[8][256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const float* dzc = dz + (int64_t)c * R;
    const float* xc = x + (int64_t)c * R;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
    for (int64_t r = tid; r < R; r += 256) {
        const int t = (int)(r % T);
        const float g = dzc[r];
        acc[7] += g;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int tt = t + j - 3;
            if (tt >= 0 && tt < T) acc[j] = fmaf(g, xc[r + j - 3], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[j][tid] = acc[j];
    __syncthreads();
    for (int wd = 128; wd > 0; wd >>= 1) {
        if (tid < wd) {
#pragma unroll
            for (int j = 0; j < 8; ++j) red[j][tid] += red[j][tid + wd];
        }
        __syncthreads();
    }
    if (tid < 7) dw[c * 7 + tid] = red[tid][0];
    if (tid == 7) db[c] = red[7][0];
}

hipError_t launch_vt_dwconv7(const float* x, const float* w, const float* bias, float* z, int C, int B, int T, hipStream_t s) {
    const int64_t R = (int64_t)B * T, n = (int64_t)C * R;
    hipLaunchKernelGGL(vt_dwconv7_kernel, dim3(grid_1d(n, 8192)), dim3(256), 0, s, x, w, bias, z, T, R, n);
    return hipGetLastError();
}

hipError_t launch_vt_dwconv7_bwd(const float* dz, const float* x, const float* w, const float* dres, float* dx, float* dw, float* db,
                                 int C, int B, int T, hipStream_t s) {
    const int64_t R = (int64_t)B * T, n = (int64_t)C * R;
    hipLaunchKernelGGL(vt_dwconv7_dx_kernel, dim3(grid_1d(n, 8192)), dim3(256), 0, s, dz, w, dres, dx, T, R, n);
    hipLaunchKernelGGL(vt_dwconv7_param_kernel, dim3(C), dim3(256), 0, s, dz, x, dw, db, T, R);
    return hipGetLastError();
}

// ---------------------------------------------------------------- exact GELU (nn.GELU(), module.py:39)
__global__ __launch_bounds__(256) void vt_gelu_kernel(const float* __restrict__ u, float* __restrict__ g, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = u[i];
        g[i] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    }
}

// gelu'(u) = Phi(u) + u phi(u): Phi = (1 + erf(u / sqrt 2)) / 2, phi = exp(-u^2 / 2) / sqrt(2 pi)
__global__ __launch_bounds__(256) void vt_gelu_bwd_kernel(const float* dg, const float* __restrict__ u, float* du, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = u[i];
        const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752440f));
        const float pdf = expf(-0.5f * v * v) * 0.39894228040143267794f;
        du[i] = dg[i] * (cdf + v * pdf);
    }
}

hipError_t launch_vt_gelu(const float* u, float* g, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(vt_gelu_kernel, dim3(grid_1d(n, 8192)), dim3(256), 0, s, u, g, n);
    return hipGetLastError();
}

hipError_t launch_vt_gelu_bwd(const float* dg, const float* u, float* du, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(vt_gelu_bwd_kernel, dim3(grid_1d(n, 8192)), dim3(256), 0, s, dg, u, du, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------- layer scale + residual (module.py:41-45)
__global__ __launch_bounds__(256) void vt_scale_residual_kernel(const float* __restrict__ xi, const float* __restrict__ y2, const float* __restrict__ gamma,
                                                                float* __restrict__ xo, int64_t R, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        xo[i] = fmaf(gamma[i / R], y2[i], xi[i]);
}

__global__ __launch_bounds__(256) void vt_scale_bwd_kernel(const float* __restrict__ dx, const float* __restrict__ y2, const float* __restrict__ gamma,
                                                           float* __restrict__ dy2, float* __restrict__ dgamma, int64_t R) {
    __shared__ float red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const float gm = gamma[c];
    const int64_t base = (int64_t)c * R;
    float acc = 0.0f;
    for (int64_t r = tid; r < R; r += 256) {
        const float g = dx[base + r];
        acc = fmaf(g, y2[base + r], acc);
        dy2[base + r] = gm * g;
    }
    const float sum = block_sum256(red, acc);
    if (tid == 0) dgamma[c] = sum;
}

hipError_t launch_vt_scale_residual(const float* xi, const float* y2, const float* gamma, float* xo, int C, int64_t R, hipStream_t s) {
    const int64_t n = (int64_t)C * R;
    hipLaunchKernelGGL(vt_scale_residual_kernel, dim3(grid_1d(n, 8192)), dim3(256), 0, s, xi, y2, gamma, xo, R, n);
    return hipGetLastError();
}

hipError_t launch_vt_scale_bwd(const float* dx, const float* y2, const float* gamma, float* dy2, float* dgamma, int C, int64_t R, hipStream_t s) {
    hipLaunchKernelGGL(vt_scale_bwd_kernel, dim3(C), dim3(256), 0, s, dx, y2, gamma, dy2, dgamma, R);
    return hipGetLastError();
}

// ---------------------------------------------------------------- transpose through a 32 x 33 LDS tile
__global__ __launch_bounds__(256) void vt_transpose_kernel(const float* __restrict__ src, int64_t rows, int cols, int64_t src_pitch,
                                                           float* __restrict__ dst, int64_t dst_pitch) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    for (int k = ty; k < 32; k += 8) {
        const int64_t r = r0 + k;
        const int c = c0 + tx;
        tile[k][tx] = (r < rows && c < cols) ? src[r * src_pitch + c] : 0.0f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k;
        const int64_t r = r0 + tx;
        if (r < rows && c < cols) dst[(int64_t)c * dst_pitch + r] = tile[tx][k];
    }
}

hipError_t launch_vt_transpose(const float* src, int64_t rows, int cols, int64_t src_pitch, float* dst, int64_t dst_pitch, hipStream_t s) {
    if (rows < 1 || cols < 1) return hipErrorInvalidValue;
    const int64_t gx = (rows + 31) / 32;
    const int gy = (cols + 31) / 32;
    if (gx > 0x7fffffff || gy > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vt_transpose_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, src, rows, cols, src_pitch, dst, dst_pitch);
    return hipGetLastError();
}

// ---------------------------------------------------------------- ISTFT head backward
// One block (256 threads) per frame.  The frame's gradient df[n] = w[n] g[m - 768] / env[m], m = t * 512 + n, is gathered from
// d audio (the forward's overlap-add read backwards: each output sample divides by the envelope of the frames that cover it, summed
// in the forward's ascending frame order).  F = rfft(df) is ONE complex FFT of 1024 points on z[n] = df[2n] + i df[2n+1]:
// the forward transform is the conjugate of voc_spec_ifft_kernel's inverse passes applied to conj z (5 radix-4 Stockham
// passes between two LDS buffers), then the split pass
//     F[k] = E - i e^{-2 pi i k / 2048} O,   E = (Z[k] + conj Z[1024-k]) / 2,   O = (Z[k] - conj Z[1024-k]) / 2.
// irfft (norm "backward") is x[n] = (1 / N) sum_k c_k (Re_k cos - Im_k sin)(2 pi k n / N) with c = 1 at k = 0, N / 2 (whose
// imaginary parts it ignores) and 2 elsewhere, hence dRe_k = c_k / N Re F_k and dIm_k = c_k / N Im F_k; S = mag e^{ip} gives the rest.
__device__ __forceinline__ float2 vt_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

__global__ __launch_bounds__(256) void vt_istft_bwd_kernel(const float* __restrict__ g, const float* __restrict__ window,
                                                           const float* __restrict__ hrows, float* __restrict__ dhrows, int T) {
    __shared__ float2 bufA[1024 + 8], bufB[1024 + 8], tw[1024];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int64_t b = row / T;
    const int t = (int)(row - b * T);
    const int64_t len = (int64_t)T * kVocHop;
    const int pad = (kVocNfft - kVocHop) / 2;
    const float* gb = g + b * len;
    for (int k = tid; k < 1024; k += 256) {
        float sn, cs;
        sincospif((float)k * (1.0f / 512.0f), &sn, &cs);         // e^{+2 pi i k / 1024}
        tw[k] = make_float2(cs, sn);
    }
    for (int n2 = tid; n2 < 1024; n2 += 256) {
        float v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = 2 * n2 + h;
            const int64_t q = (int64_t)t * kVocHop + n;           // position in the untrimmed signal
            float d = 0.0f;
            if (q >= pad && q < pad + len) {
                int f1 = (int)(q / kVocHop); if (f1 > T - 1) f1 = T - 1;
                int64_t f0 = (q - (kVocNfft - 1) + kVocHop - 1) / kVocHop; if (q - (kVocNfft - 1) < 0) f0 = 0;
                float env = 0.0f;
                for (int f = (int)f0; f <= f1; ++f) {
                    const float wv = window[(int)(q - (int64_t)f * kVocHop)];
                    env += wv * wv;
                }
                d = window[n] * (gb[q - pad] / env);
            }
            v[h] = d;
        }
        bufA[n2] = make_float2(v[0], -v[1]);                      // conj z
    }
    __syncthreads();
    float2* in = bufA; float2* out = bufB;
#pragma unroll 1
    for (int Ns = 1; Ns < 1024; Ns <<= 2) {
        const int j = tid, k = j & (Ns - 1);
        const int tstep = k * (256 / Ns);
        const float2 u0 = in[j];
        const float2 u1 = vt_cmul(in[j + 256], tw[tstep]);
        const float2 u2 = vt_cmul(in[j + 512], tw[2 * tstep]);
        const float2 u3 = vt_cmul(in[j + 768], tw[3 * tstep]);
        const float2 s02 = make_float2(u0.x + u2.x, u0.y + u2.y), d02 = make_float2(u0.x - u2.x, u0.y - u2.y);
        const float2 s13 = make_float2(u1.x + u3.x, u1.y + u3.y), d13 = make_float2(u1.x - u3.x, u1.y - u3.y);
        const int j0 = ((j - k) << 2) + k;
        out[j0] = make_float2(s02.x + s13.x, s02.y + s13.y);
        out[j0 + Ns] = make_float2(d02.x - d13.y, d02.y + d13.x);
        out[j0 + 2 * Ns] = make_float2(s02.x - s13.x, s02.y - s13.y);
        out[j0 + 3 * Ns] = make_float2(d02.x + d13.y, d02.y - d13.x);
        __syncthreads();
        float2* tmp = in; in = out; out = tmp;
    }
    // in[k] = conj Z[k]
    const float* hr = hrows + row * (2 * kVocHeadPlane);
    float* dr = dhrows + row * (2 * kVocHeadPlane);
    for (int k = tid; k <= 1024; k += 256) {
        const float2 ca = in[k & 1023], cb = in[(1024 - k) & 1023];
        const float2 A = make_float2(ca.x, -ca.y), Bz = make_float2(cb.x, -cb.y);
        const float2 E = make_float2(0.5f * (A.x + Bz.x), 0.5f * (A.y - Bz.y));
        const float2 O = make_float2(0.5f * (A.x - Bz.x), 0.5f * (A.y + Bz.y));
        float sn, cs;
        sincospif((float)k * (1.0f / 1024.0f), &sn, &cs);
        const float2 P = vt_cmul(make_float2(cs, -sn), O);        // e^{-2 pi i k / 2048} O
        const bool edge = k == 0 || k == 1024;
        const float ck = edge ? (1.0f / 2048.0f) : (2.0f / 2048.0f);
        const float dRe = ck * (E.x + P.y);
        const float dIm = edge ? 0.0f : ck * (E.y - P.x);
        const float ea = expf(hr[k]);
        const float mag = fminf(ea, 100.0f);                      // head.py:105-106
        float ps, pc;
        sincosf(hr[kVocHeadPlane + k], &ps, &pc);
        dr[k] = ea <= 100.0f ? mag * (dRe * pc + dIm * ps) : 0.0f;        // torch.clip passes the gradient where exp(a) <= max
        dr[kVocHeadPlane + k] = mag * (dIm * pc - dRe * ps);
    }
}

hipError_t launch_vt_istft_bwd(const float* g, const float* window, const float* hrows, float* dhrows, int B, int T, hipStream_t s) {
    const int64_t rows = (int64_t)B * T;
    if (rows < 1 || rows > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vt_istft_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, s, g, window, hrows, dhrows, T);
    return hipGetLastError();
}

}  // namespace st
