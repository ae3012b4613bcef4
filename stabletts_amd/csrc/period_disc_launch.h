// Launcher interface of the period-discriminator kernels (period_disc_kernels.hip).
// Reference: vocoders/vocos/models/discriminator.py:32-75 (DiscriminatorP).  Everything is fp32 and keeps the reference's
// layout (B, C, H, p) contiguous, p = the period: a frame of an item is n = h * p + w, and a (k, 1) conv with stride (s, 1) is a
// strided 1-D conv over h with B * p independent columns.  Tap j of output (h, w) reads input frame (s h + j - taps/2) p + w,
// zero where that row is outside [0, Hin).  The GEMMs of layers 1-4 run on the fp32-input MFMA with the 64 x 64 tile of
// style_dp_kernels.hip; layer 0 (Cin = 1), conv_post (Cout = 1) and the weight norm are VALU kernels.  No atomics: every
// reduction has a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace st {

constexpr int kPdTaps = 5, kPdPostTaps = 3, kPdC0 = 32;

// Forward of layers 1-4: out[b][co][h][w] = lrelu(bias[co] + sum_{ci, j} w[co][ci][j] in[b][ci][stride h + j - 2][w]);
// in (B, Cin, Hin, p), w (Cout, Cin, 5), out (B, Cout, Hout, p); out2 (nullable) receives the same values.
// Data gradient (launch_pd_conv_dgrad): in = dY (B, Cin = Cout_fwd, Hin = Hout_fwd, p), out = d pre-activation of the layer
// below (B, Cout = Cin_fwd, Hout = Hin_fwd, p):
//   out = (sum_{co, j : stride ho + j - 2 = hi} w[co][ci][j] dY[b][co][ho][w] + (addg ? addg : 0)) * (act > 0 ? 1 : slope)
// act: the kept POST-activation of the layer below (with slope > 0 its sign is the pre-activation's), addg: the gradient that
// reaches that activation from outside (its feature map), both in out's layout.  With stride 3 an input row takes one or two
// of the five taps: the launch runs one tile family per residue class of (hi + 2) % 3, each over its own taps only.
struct PdConvArgs {
    const float* in = nullptr; const float* w = nullptr; const float* bias = nullptr;
    float* out = nullptr; float* out2 = nullptr;
    const float* act = nullptr; const float* addg = nullptr;
    int B = 0, Cin = 0, Cout = 0, Hin = 0, Hout = 0, p = 1, stride = 1;
    float slope = 0.1f;
};
hipError_t launch_pd_conv(const PdConvArgs& a, hipStream_t s);
hipError_t launch_pd_conv_dgrad(const PdConvArgs& a, hipStream_t s);

// Weight gradient of layers 1-4: dw[co][ci][j] = sum_{b, h, w} dy[b][co][h][w] in[b][ci][stride h + j - 2][w]; a TN GEMM over
// K = B * Hout * p frames, split into fixed frame ranges whose planes are summed in a fixed order (as launch_sd_wgrad).
struct PdWgradArgs {
    const float* dy = nullptr; const float* in = nullptr; float* dw = nullptr; float* scratch = nullptr;
    int B = 0, Cin = 0, Cout = 0, Hin = 0, Hout = 0, p = 1, stride = 1;
};
size_t pd_wgrad_scratch_floats(int B, int Cin, int Cout, int Hout, int p);
int pd_wgrad_planes(int B, int Cin, int Cout, int Hout, int p);          // split-K planes of that launch (tests / tools)
hipError_t launch_pd_wgrad(const PdWgradArgs& a, hipStream_t s);

// Layer 0 (Cin = 1, 32 channels, 5 taps, stride 3) on the waveform x (B, T), with the reference's tail padding
// (F.pad(x, (0, Tp - T), "reflect"): padded sample n >= T is x[2 (T - 1) - n]) and the leaky ReLU: out (B, 32, H0, p).
hipError_t launch_pd_l0_fwd(const float* x, const float* w, const float* bias, float* out, int B, int T, int Tp, int H0, int p, float slope,
                            hipStream_t s);
// dw (32, 5) and db (32) from dpre (B, 32, H0, p): per-range partial sums (scratch: pd_l0_scratch_floats) added in a fixed order
size_t pd_l0_scratch_floats(int B, int H0, int p);
hipError_t launch_pd_l0_wgrad(const float* dpre, const float* x, float* dw, float* db, float* scratch, int B, int T, int Tp, int H0, int p,
                              hipStream_t s);
// dx (B, T): the gradient of the padded waveform with the padded samples' share folded back onto the samples they mirror
hipError_t launch_pd_l0_dgrad(const float* dpre, const float* w, float* dx, int B, int T, int Tp, int H0, int p, hipStream_t s);

// conv_post (C -> 1, 3 taps, stride 1, no activation): out[b][h][w] = bias + sum_{ci, j} w[ci][j] in[b][ci][h + j - 1][w], the
// channels reduced in a fixed order; out2 nullable.  Its data gradient is the outer product
//   dpre[b][ci][h][w] = (sum_j w[ci][j] dy[b][h + 1 - j][w] + (addg ? addg : 0)) * (act > 0 ? 1 : slope)      (dy nullable: 0)
// and its weight gradient a per-channel dot product dw[ci][j] = sum_{b, h, w} dy[b][h][w] in[b][ci][h + j - 1][w].
hipError_t launch_pd_post_fwd(const float* in, const float* w, const float* bias, float* out, float* out2, int B, int C, int H, int p,
                              hipStream_t s);
hipError_t launch_pd_post_dgrad(const float* dy, const float* w, const float* act, const float* addg, float* dpre, int B, int C, int H, int p,
                                float slope, hipStream_t s);
hipError_t launch_pd_post_wgrad(const float* dy, const float* in, float* dw, int B, int C, int H, int p, hipStream_t s);

// Weight norm over dim 0 (torch.nn.utils.parametrizations.weight_norm): w[co][:] = v[co][:] g[co] / ||v[co][:]||, one block per
// output channel; backward: dg = <dw, v> / ||v||, dv = (g / ||v||) (dw - v dg / ||v||).  n = elements per output channel.
hipError_t launch_pd_weight_norm(const float* v, const float* g, float* w, int Cout, int n, hipStream_t s);
hipError_t launch_pd_weight_norm_bwd(const float* dw, const float* v, const float* g, float* dv, float* dg, int Cout, int n, hipStream_t s);

}  // namespace st
