// Launcher interface of the MelStyleEncoder and DurationPredictor kernels (style_dp_kernels.hip).
// Reference: models/reference_encoder.py:22-93 (MelStyleEncoder, Conv1dGLU), models/duration_predictor.py:5-37.
// Everything is fp32 and channel-major (B, C, T), the reference's own layout: the GEMMs run on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32, an exact k-ordered fp32 FMA chain), the row work on the VALU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace st {

enum SdEpi { SD_EPI_NONE = 0, SD_EPI_MISH = 1, SD_EPI_RELU = 2 };

// out[b][co][t] = epi(bias[co] + sum_{ci, j} W[co][ci][j] * x'[b][ci][t + j - taps/2]) * (omask ? omask[b][t] : 1)
//   x'[b][ci][t] = (in[b][ci][t] + (addv ? addv[b][ci] : 0)) * (imask ? imask[b][t] : 1), zero outside [0, T).
// in (B, Cin, T), W (Cout, Cin, taps) as nn.Conv1d / nn.Linear store it (taps 1, 3 or 5), out (B, Cout, T); masks (B, T).
struct SdConvArgs {
    const float* in = nullptr; const float* addv = nullptr; const float* imask = nullptr;
    const float* w = nullptr; const float* bias = nullptr; const float* omask = nullptr;
    float* out = nullptr;
    int B = 0, Cin = 0, Cout = 0, T = 0, taps = 1, epi = SD_EPI_NONE;
};
hipError_t launch_sd_conv(const SdConvArgs& a, hipStream_t s);

// Conv1dGLU's tail (reference_encoder.py:17-20): h[b][c][t] += u[b][c][t] * sigmoid(u[b][C + c][t]);  u (B, 2C, T), h (B, C, T)
hipError_t launch_sd_glu_residual(float* h, const float* u, int B, int C, int T, hipStream_t s);

// nn.LayerNorm(C) over the channels of every frame of x (B, C, T), in place (duration_predictor.py:28,32)
hipError_t launch_sd_layernorm_channels(float* x, const float* w, const float* b, float eps, int B, int C, int T, hipStream_t s);

// nn.MultiheadAttention's core for head_dim 64 without RoPE: qkv (B, 3 * H * 64, T) = [q | k | v] channel planes of in_proj,
// out (B, H * 64, T).  Key t of item b takes part iff kmask == nullptr or kmask[b][t] != 0 (key_padding_mask); a query with
// no valid key writes 0.
hipError_t launch_sd_attention(const float* qkv, const float* kmask, float* out, int B, int H, int T, hipStream_t s);

// c[b][o] = mean over the frames t with (mask == nullptr || mask[b][t] != 0) of x[b][o][t]; NaN when there is none
// (reference_encoder.py:68-72); x (B, O, T), c (B, O)
hipError_t launch_sd_mean_pool(const float* x, const float* mask, float* c, int B, int O, int T, hipStream_t s);

}  // namespace st
