// Launcher interface of the MelStyleEncoder and DurationPredictor kernels (style_dp_kernels.hip).
// Reference: models/reference_encoder.py:22-93 (MelStyleEncoder, Conv1dGLU), models/duration_predictor.py:5-37.
// Everything is fp32 and channel-major (B, C, T), the reference's own layout: the GEMMs run on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32, an exact k-ordered fp32 FMA chain), the row work on the VALU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace st {

// Dropout of one training site (style_dp_bwd.hip): the decoder's counter-based hash (common.h) with the salted seed words of
// make_drop (train_kernels.hip); thresh16 == 0: keep everything with factor 1.  The masks are recomputed in the backward.
struct SdDrop { unsigned long long seed = 0; unsigned thresh16 = 0; float scale = 1.0f; };
SdDrop sd_make_drop(float p, unsigned long long seed, int salt);
// (device side of the masks: style_dp_drop.h)

enum SdEpi { SD_EPI_NONE = 0, SD_EPI_MISH = 1, SD_EPI_RELU = 2 };

// out[b][co][t] = epi(bias[co] + sum_{ci, j} W[co][ci][j] * x'[b][ci][t + j - taps/2]) * (omask ? omask[b][t] : 1)
//   x'[b][ci][t] = (in[b][ci][t] + (addv ? addv[b][ci] : 0)) * (imask ? imask[b][t] : 1), zero outside [0, T).
// in (B, Cin, T), W (Cout, Cin, taps) as nn.Conv1d / nn.Linear store it (taps 1, 3 or 5), out (B, Cout, T); masks (B, T).
struct SdConvArgs {
    const float* in = nullptr; const float* addv = nullptr; const float* imask = nullptr;
    const float* w = nullptr; const float* bias = nullptr; const float* omask = nullptr;
    float* out = nullptr;
    int B = 0, Cin = 0, Cout = 0, T = 0, taps = 1, epi = SD_EPI_NONE;
    int chains = 1;                  // launch_sd_conv / _dgrad, taps = 1: 4 = four interleaved accumulation chains over K (sd_conv_kernel)
    const float* res = nullptr;      // launch_sd_conv_dgrad only: added to the (masked) output, layout of out
    float* pre = nullptr;            // launch_sd_conv_pre only: receives bias + sum (the pre-activation), layout of out
};
enum SdConvMode { SD_MODE_FWD = 0, SD_MODE_DGRAD = 1, SD_MODE_FWD_PRE = 2 };      // sd_conv_kernel's template modes
hipError_t launch_sd_conv(const SdConvArgs& a, hipStream_t s);

// launch_sd_conv that also writes the pre-activation (bias + sum, before epi and omask) to a.pre: the training forward keeps
// it for the activation's backward while `out` stays bitwise the inference value
hipError_t launch_sd_conv_pre(const SdConvArgs& a, hipStream_t s);

// ---- training (style_dp_bwd.hip) ----------------------------------------------------------------------------------------
// Data gradient of a conv with nn.Conv1d weight w (Cout_fwd, Cin_fwd, taps): in = dY (B, Cin = Cout_fwd, T), out = dX
// (B, Cout = Cin_fwd, T): out[b][ci][t] = omask[b][t] * sum_{co, j} w[co][ci][j] dY[b][co][t - j + taps/2] (+ res).
// The same tile kernel as launch_sd_conv (template DGRAD); bias, addv, imask and epi are not used.
hipError_t launch_sd_conv_dgrad(const SdConvArgs& a, hipStream_t s);

// Weight gradient dW[co][ci][j] = sum_{b, t} dY[b][co][t] x'[b][ci][t + j - taps/2], x' as in SdConvArgs (in, addv, imask).
// A TN GEMM over K = B * T frames on the fp32 MFMA, split into fixed frame ranges written to planes of `scratch`, the planes
// summed in a fixed order: no atomics, bitwise reproducible.  scratch: sd_wgrad_scratch_floats() floats.
struct SdWgradArgs {
    const float* dy = nullptr; const float* in = nullptr; const float* addv = nullptr; const float* imask = nullptr;
    float* dw = nullptr; float* scratch = nullptr;
    int B = 0, Cin = 0, Cout = 0, T = 0, taps = 1;
};
size_t sd_wgrad_scratch_floats(int B, int Cin, int Cout, int T, int taps);
hipError_t launch_sd_wgrad(const SdWgradArgs& a, hipStream_t s);

// out[c] (per_item = 0) or out[b][c] (per_item = 1) = sum over t (and b) of x[b][c][t]: bias gradients, d cond; fixed order.
hipError_t launch_sd_sum_frames(const float* x, float* out, int B, int C, int T, int per_item, hipStream_t s);
// y = x * mask[b][t] (mask (B, T)), x / y (B, C, T); in place allowed
hipError_t launch_sd_mul_mask(const float* x, const float* mask, float* y, int B, int C, int T, hipStream_t s);

// Element-site dropout in place: x[i] *= keep factor of element i (x: n elements)
hipError_t launch_sd_drop(float* x, const SdDrop& d, int64_t n, hipStream_t s);
// Mish backward from the kept pre-activation: dpre = dout * keep * mish'(pre)
hipError_t launch_sd_mish_bwd(const float* dout, const float* pre, float* dpre, const SdDrop& d, int64_t n, hipStream_t s);

// Conv1dGLU's tail with dropout on the gated product: hout = hin + value * sigmoid(gate) * keep (u (B, 2C, T) = [value | gate]);
// backward: du = [dh * keep * sigmoid(gate) | dh * keep * value * sigmoid (1 - sigmoid)] (the residual passes dh through)
hipError_t launch_sd_glu_train(const float* hin, const float* u, float* hout, const SdDrop& d, int B, int C, int T, hipStream_t s);
hipError_t launch_sd_glu_bwd(const float* dh, const float* u, float* du, const SdDrop& d, int B, int C, int T, hipStream_t s);

// nn.LayerNorm over the channels, out of place, + dropout: y = LN(x) * keep; mean / rstd (B, T) kept for the backward.
// The backward: dn = dy * keep, dx = rstd (dn w - mean_c(dn w) - xhat mean_c(dn w xhat)) * (x > 0 if relu_x: x is a ReLU output);
// dw[c] = sum_{b,t} dn xhat, db[c] = sum_{b,t} dn (one block per channel, fixed order).
hipError_t launch_sd_layernorm_train(const float* x, float* y, float* mean, float* rstd, const float* w, const float* b, float eps,
                                     const SdDrop& d, int B, int C, int T, hipStream_t s);
hipError_t launch_sd_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* w, float* dx,
                                   float* dw, float* db, const SdDrop& d, int relu_x, int B, int C, int T, hipStream_t s);

// launch_sd_attention plus dropout d on the probabilities; stats (2, B, H, T): each query's running max and 1 / sum
hipError_t launch_sd_attention_train(const float* qkv, const float* kmask, float* out, float* stats, const SdDrop& d, int B, int H, int T,
                                     hipStream_t s);
// Its backward: dout (B, H*64, T) -> dqkv (B, 3*H*64, T).  Pass 1 owns query tiles (dq, and D = rowsum(dO o O) into dsum
// (B, H, T)); pass 2 owns key tiles (dk, dv; exactly 0 for masked keys).  P is recomputed from stats, the dropout mask from d.
hipError_t launch_sd_attention_bwd(const float* qkv, const float* kmask, const float* out, const float* dout, const float* stats,
                                   float* dsum, float* dqkv, const SdDrop& d, int B, int H, int T, hipStream_t s);

// Masked mean-pool backward: dx[b][o][t] = dc[b][o] / n_b on frames with mask != 0 (all with mask == nullptr), else 0
hipError_t launch_sd_mean_pool_bwd(const float* dc, const float* mask, float* dx, int B, int O, int T, hipStream_t s);

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
