// Launcher interface of the Vocos training kernels (vocos_train_kernels.hip): the row work of the fp32 training forward
// and of the backward around the fp32 MFMA GEMMs of style_dp_launch.h.
// Reference: vocoders/vocos/models/backbone.py:50-56, module.py:33-46, head.py:39-72,93-117 under autograd.
// Every tensor is fp32 and channel-major over the FLATTENED frames of the batch: (C, R), R = B * T, frame r = b * T + t.
// The pointwise convs and the head mix no frames, so they run the tile kernels as B = 1, T = R; the kernels here that do
// mix frames (embed im2col, depthwise conv, ISTFT) take T and never cross an item's boundary.
// No atomics: every reduction has a fixed order, two runs give bitwise identical results.
#pragma once
#include "vocos_launch.h"

namespace st {

// cols[(ci * 7 + j) * R + b * T + t] = mel[b][ci][t + j - 3] (0 outside [0, T)): the k = 7 embed conv as a k = 1 conv with
// Cin = 7 M whose weight is backbone.embed.weight (C, M, 7) read as (C, 7 M) in place
hipError_t launch_vt_im2col7(const float* mel, float* cols, int B, int M, int T, hipStream_t s);
// dmel[b][ci][t] = sum_j dcols[(ci * 7 + j) * R + b * T + t - j + 3] over the j with 0 <= t - j + 3 < T, ascending j
hipError_t launch_vt_col2im7(const float* dcols, float* dmel, int B, int M, int T, hipStream_t s);

// z[c][r] = bias[c] + sum_j w[c][j] x[c][r + j - 3] within the item of r (nn.Conv1d(C, C, 7, padding=3, groups=C))
hipError_t launch_vt_dwconv7(const float* x, const float* w, const float* bias, float* z, int C, int B, int T, hipStream_t s);
// dx[c][r] = dres[c][r] + sum_j w[c][j] dz[c][r - j + 3] (the block's residual gradient passes through);
// dw[c][j] = sum_r dz[c][r] x[c][r + j - 3], db[c] = sum_r dz[c][r]  (one block per channel, fixed order)
hipError_t launch_vt_dwconv7_bwd(const float* dz, const float* x, const float* w, const float* dres, float* dx, float* dw, float* db,
                                 int C, int B, int T, hipStream_t s);

// exact (erf) GELU: g = gelu(u); backward from the kept pre-activation: du = dg * gelu'(u) (in place allowed)
hipError_t launch_vt_gelu(const float* u, float* g, int64_t n, hipStream_t s);
hipError_t launch_vt_gelu_bwd(const float* dg, const float* u, float* du, int64_t n, hipStream_t s);

// layer scale + residual: xo[c][r] = xi[c][r] + gamma[c] * y2[c][r];
// backward: dy2 = gamma[c] * dx, dgamma[c] = sum_r dx[c][r] y2[c][r] (one block per channel); dx itself passes through
hipError_t launch_vt_scale_residual(const float* xi, const float* y2, const float* gamma, float* xo, int C, int64_t R, hipStream_t s);
hipError_t launch_vt_scale_bwd(const float* dx, const float* y2, const float* gamma, float* dy2, float* dgamma, int C, int64_t R, hipStream_t s);

// dst[c * dst_pitch + r] = src[r * src_pitch + c], r < rows, c < cols
hipError_t launch_vt_transpose(const float* src, int64_t rows, int cols, int64_t src_pitch, float* dst, int64_t dst_pitch, hipStream_t s);

// ISTFT head backward (head.py:39-72,104-116; n_fft 2048, hop 512, padding "same").  g (B, T * 512) = d loss / d audio,
// hrows / dhrows [R][2 * kVocHeadPlane]: the head output (log-magnitude plane a, phase plane p) and its gradient.
// Per frame: df[n] = w[n] g[m - 768] / env[m] on m = t * 512 + n in [768, 768 + T * 512) (a gather), F = rfft(df) as one
// 1024-point complex FFT in LDS, dRe_k = c_k / N Re F_k, dIm_k = c_k / N Im F_k (c = 1 at k = 0 and N / 2 where dIm = 0, else 2),
// da = mag (dRe cos p + dIm sin p) where exp(a) <= 100 and exactly 0 otherwise, dp = mag (-dRe sin p + dIm cos p), mag = min(exp a, 100).
hipError_t launch_vt_istft_bwd(const float* g, const float* window, const float* hrows, float* dhrows, int B, int T, hipStream_t s);

}  // namespace st
