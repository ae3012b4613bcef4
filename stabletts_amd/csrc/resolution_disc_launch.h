// Launcher interface of the resolution-discriminator kernels (resolution_disc_kernels.hip).
// Reference: vocoders/vocos/models/discriminator.py:112-171 (DiscriminatorR).  Everything is fp32 in the reference's layout
// (B, C, frames, F) contiguous.  The complex STFT (window W, hop W / 4, reflect padding W / 2, hann window) is written as
// (B, 2, frames, W / 2 + 1): Re and Im are the two input channels of layer 0 and a band is a column range [lo, hi) of it.
// Each of the five bands runs its own stack of five convs (2 -> 32 with (3, 9) taps; three 32 -> 32 with (3, 9) taps and stride
// (1, 2); 32 -> 32 with (3, 3) taps; leaky ReLU after each); conv_post (32 -> 1, (3, 3)) reads the bands' last activations side by
// side along F.  The forward of all five layers and the data gradient of the 32 -> 32 layers are implicit GEMMs on the fp32-input
// MFMA with fp32_tile.h's 32 x 128 tile, one launch for the five bands; layer 0's data gradient (2 output channels), conv_post and
// the STFT are vector kernels; the weight gradients go through fp32_tile.h's split-K kernel.  No atomics: every reduction has a
// fixed order, and an item's values do not depend on the rest of its batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace st {

constexpr int kRdBands = 5, kRdCh = 32, kRdRows = 3;      // bands; channels of every band conv; taps along the frames of every conv

// ---- complex STFT ------------------------------------------------------------------------------------------------------------
// spec[b][0 / 1][t][k] = Re / Im of sum_n w[n] x[s(t hop + n - W / 2)] e^{-2 pi i k n / W}, s = torch's reflect index.  x (B, T).
hipError_t launch_rd_stft(const float* x, const float* window, float* spec, int W, int B, int T, int frames, hipStream_t s);
// d x (B, T) from d spec (B, 2, frames, W / 2 + 1): per frame w[n] Re sum_k (dRe_k + i dIm_k) e^{+2 pi i k n / W} into ws
// (B, frames, W floats), then audio_kernels.hip's gather onto the samples, reflected ones folded back.
hipError_t launch_rd_stft_backward(const float* dspec, const float* window, float* ws, float* dx, int W, int B, int T, int frames, hipStream_t s);

// ---- band convs ----------------------------------------------------------------------------------------------------------------
// One band of a launch.  Forward: out[b][co][t][f] = lrelu(bias[co] + sum_{ci, jt, jf} w[co][ci][jt][jf] in[b][ci][t + jt - 1][sw f + jf - pw]),
// f < Wout, zero outside [0, frames) x [0, Win); `in` has row stride in_rs (the spectrum: W / 2 + 1, `in` pointing at column lo; an
// activation: Win), out / out2 (nullable, the same values) are dense (B, Cout, frames, Wout).
// Data gradient: in = dY (B, Cin = the forward's Cout, frames, Win = the forward's Wout), out = d pre-activation of the layer below,
// dense (B, Cout, frames, Wout = the forward's Win):
//   out = (sum_{co, jt, jf : sw fo + jf - pw = fi} w[co][ci][jt][jf] dY[b][co][t + 1 - jt][fo] + (addg ? addg : 0)) * (act > 0 ? 1 : slope)
// act: the kept POST-activation of the layer below, addg: the gradient reaching it from outside (its feature map).
struct RdBand {
    const float* in = nullptr; const float* w = nullptr; const float* bias = nullptr;
    float* out = nullptr; float* out2 = nullptr;
    const float* act = nullptr; const float* addg = nullptr;
    int in_rs = 0, Win = 0, Wout = 0;
};
struct RdConvArgs {
    RdBand band[kRdBands];
    int B = 0, Cin = 0, Cout = 0, frames = 0;
    int taps_w = 9;          // 9: padding 4; 3: padding 1
    int stride_w = 1;        // 1 or 2 (taps_w = 9 only)
    float slope = 0.1f;
};
hipError_t launch_rd_conv(const RdConvArgs& a, hipStream_t s);
// stride 2: one tile family per parity of the input column (even columns take taps 0, 2, .. 8, odd ones 1, 3, 5, 7), a launch each
hipError_t launch_rd_conv_dgrad(const RdConvArgs& a, hipStream_t s);

// Weight gradient of one band conv: dw[co][ci][jt][jf] = sum_{b, t, f} dy[b][co][t][f] in[b][ci][t + jt - 1][sw f + jf - pw]; a TN GEMM
// over B * frames * Wout frames, split into fixed ranges whose planes are summed in a fixed order.
struct RdWgradArgs {
    const float* dy = nullptr; const float* in = nullptr; float* dw = nullptr; float* scratch = nullptr;
    int B = 0, Cin = 0, frames = 0, in_rs = 0, Win = 0, Wout = 0, taps_w = 9, stride_w = 1;
};
size_t rd_wgrad_scratch_floats(int B, int Cin, int frames, int Wout, int taps_w);
int rd_wgrad_planes(int B, int Cin, int frames, int Wout, int taps_w);       // split-K planes of that launch (tests / tools)
hipError_t launch_rd_wgrad(const RdWgradArgs& a, hipStream_t s);

// Bias gradients of one layer, the five bands in one launch: db[c][co] = sum_{b, t, f} d[c][b][co][t][f], d[c] (B, 32, frames, width[c]).
// Two stages with a fixed order: every (band, channel) sums position ranges (an LDS tree each; their number follows from the widest
// band) into `part` (rd_bias_scratch_floats() floats for bands up to `widest` columns), then one thread per (band, channel) adds
// its ranges in order.
struct RdBiasArgs {
    const float* d[kRdBands]; float* db[kRdBands];
    int width[kRdBands];
    float* part = nullptr;
    int B = 0, frames = 0;
};
size_t rd_bias_scratch_floats(int B, int frames, int widest);
hipError_t launch_rd_bias_grad(const RdBiasArgs& a, hipStream_t s);

// Layer 0's data gradient onto the spectrum: dspec[b][c][t][k] = sum over the bands with lo <= k < hi (in band order) of
// sum_{co, jt, jf} w[co][c][jt][jf] d0[b][co][t + 1 - jt][k - lo + 4 - jf]; bins outside every band get 0.  d0: (B, 32, frames, hi - lo).
struct RdL0DgradArgs {
    const float* d0[kRdBands]; const float* w[kRdBands];
    int lo[kRdBands], hi[kRdBands];
    float* dspec = nullptr;
    int B = 0, frames = 0, bins = 0;
};
hipError_t launch_rd_l0_dgrad(const RdL0DgradArgs& a, hipStream_t s);

// ---- conv_post (32 -> 1, (3, 3), padding 1, no activation) on the bands' layer-4 activations side by side -------------------------
// Column fc of the concatenation is column fc - off[c] of band c, off[c] <= fc < off[c + 1]; off[5] = its width Wc.
struct RdPostArgs {
    const float* in[kRdBands];            // (B, 32, frames, off[c + 1] - off[c]) each: the activations (forward, weight gradient, act)
    const float* addg[kRdBands];          // data gradient: what reaches the activation from outside, nullable each
    float* dpre[kRdBands];                // data gradient: d pre-activation of layer 4, each of in[c]'s shape
    int off[kRdBands + 1];
    const float* w = nullptr; const float* bias = nullptr;       // (32, 3, 3), (1)
    const float* dy = nullptr;            // (B, 1, frames, Wc), nullable in the data gradient (0)
    float* out = nullptr; float* out2 = nullptr;                  // forward (B, 1, frames, Wc); out2 nullable
    float* dw = nullptr;                  // weight gradient (32, 3, 3)
    float* part = nullptr;                // weight gradient: rd_post_wgrad_scratch_floats() floats of position-range partial sums
    int B = 0, frames = 0;
    float slope = 0.1f;
};
hipError_t launch_rd_post_fwd(const RdPostArgs& a, hipStream_t s);
hipError_t launch_rd_post_dgrad(const RdPostArgs& a, hipStream_t s);
size_t rd_post_wgrad_scratch_floats(int B, int frames, int Wc);
hipError_t launch_rd_post_wgrad(const RdPostArgs& a, hipStream_t s);      // position ranges summed per block, then added in range order

}  // namespace st
