// Launcher interface of the FireflyGAN vocoder kernels (ffgan_kernels.hip): the row kernels of the ConvNeXt encoder at a
// run-time width (its GEMMs reuse the implicit-GEMM kernels of launch.h, as the Vocos engine does) and the convolution
// family of the HiFi-GAN head.  Reference: vocoders/ffgan/backbone.py:146-214, head.py:25-133,136-249 (use_template=False).
// Activations are time-major [item][L][C]; fp32 residual stream, 16-bit MFMA operands, fp32 accumulation.
#pragma once
#include "launch.h"
#include "vocos_launch.h"

namespace st {

// ---------------------------------------------------------------- encoder row kernels, width C a multiple of 128 up to kFfgMaxDim
constexpr int kFfgMaxDim = 1024;
// y = LayerNorm_C(x) * w + b (eps 1e-6, biased variance) per frame: out32 and/or out16 (out32 may alias x)
hipError_t launch_ffg_ln(int dtype, const float* x, const float* w, const float* b, int64_t rows, int C, float* out32, void* out16, hipStream_t s);
// h16 = LayerNorm_C(dwconv7(x) + bias) * w + b per utterance (zero padding, rows of different items never mix); dw: [C][7]
hipError_t launch_ffg_dwconv_ln(int dtype, const float* x, const float* dw, const float* dbias, const float* w, const float* b,
                                int B, int T, int C, void* h16, hipStream_t s);
// launch_ffg_dwconv_ln on the packed rows of a ragged batch (vocos_launch.h): frames[r] names packed row r's utterance (the group
// table of launch_voc_segments at one frame per group), so a window never leaves its utterance; the arithmetic per row is the
// dense kernel's
hipError_t launch_ffg_dwconv_ln_ragged(int dtype, const float* x, const float* dw, const float* dbias, const float* w, const float* b,
                                       const VocSeg* frames, int64_t rows, int C, void* h16, hipStream_t s);

// ---------------------------------------------------------------- head: implicit-GEMM convolution on the 16x16x32 MFMA
//   out[t][co] = bias[co] + sum_j sum_ci W[co][j][ci] * a[t + (j - taps/2) * dil][ci],   a = 0 outside [0, L) of its own item
// One block = kFfgFrames frames x CW * 16 output channels (CW = 1, 2 or 4, the widest that divides cout / 16): the weights are the
// MFMA's A operand (16 output channels), the frames its B operand (16 frames), so a 16- or 32-channel level fills every wave.
// The input patch (tile + 2 * halo rows, halo = (taps / 2) * dil <= kFfgMaxHalo) of one cin chunk (kc = min(cin, 128) channels)
// is staged once in LDS as 16-bit rows and the taps are row offsets into it.  The K order of a chunk is (tap, channel), padded
// with zero weights to a multiple of 32.  Every offset into a tensor is 64-bit.
constexpr int kFfgFrames = 128;
constexpr int kFfgMaxHalo = 25;
constexpr int kFfgMaxTaps = 13;
enum { FFG_F32 = 0,        // out32 = acc + bias                                                    (conv_pre, the transposed convs)
       FFG_SILU16 = 1,     // out16 = round16(silu(acc + bias))                                     (c1 of a ResBlock pair: the operand of c2)
       FFG_RES = 2 };      // y = acc + bias + res32; out32 = y (if set); mean (if set): see below   (c2 of a pair)
struct FfgConvArgs {
    const float* in32;      // fp32 input [items][L][cin]: SiLU is applied in fp32 while staging, before the rounding to 16 bits ...
    const void* in16;       // ... or a 16-bit operand that is staged as it is (exactly one of the two is set)
    const void* wfrag;      // weights in fragment order (launch_ffg_pack_conv)
    const float* bias;      // [cout]
    int cin, cout, taps, dil, L, n_items;
    int epi;
    float* out32; void* out16;      // [items][L][cout]
    const float* res32;             // FFG_RES: the residual (may alias out32)
    // FFG_RES, the last c2 of a ResBlock: its share of the ParralelBlock mean, in block order on one stream.
    // mean = (mean_first ? y : mean + y) * mean_scale  (mean_scale = 1 / n_blocks at the last block, else 1)
    float* mean; int mean_first; float mean_scale;
    // Ragged batch (utt set): every tensor holds packed rows, item b its frames utt[b].row0 * up .. + utt[b].T * up (up: the product
    // of the upsample rates before this level) and L is the level length of the LONGEST item: it sizes the grid, a block past its own
    // item's end exits, and the patch is zero outside its own item.  Each tile then runs the arithmetic of the dense call on its item alone.
    const VocUtt* utt; int up;
};
inline int ffg_kc(int cin) { return cin < 128 ? cin : 128; }
inline int ffg_ksteps(int cin, int taps) { const int kc = ffg_kc(cin); return (cin / kc) * ((taps * kc + 31) / 32); }
inline size_t ffg_frag_bytes(int cout, int cin, int taps) { return (size_t)(cout / 16) * ffg_ksteps(cin, taps) * 1024; }
// cin: 16, 32, 64 or a multiple of 128; cout a multiple of 16; taps odd <= kFfgMaxTaps; halo <= kFfgMaxHalo
bool ffg_conv_supported(int cin, int cout, int taps, int dil);
hipError_t launch_ffg_conv(int dtype, const FfgConvArgs& a, hipStream_t s);

// scale[r] = g[r] / ||v[r, :]||_2 over the `inner` elements of row r (weight norm over all dims but 0)
hipError_t launch_ffg_wn_scale(const float* v, const float* g, int rows, int inner, float* scale, hipStream_t s);
// Fragment-ordered 16-bit weights of one convolution from the weight-norm direction v and scale (scale == nullptr: v is the weight).
//   transposed == 0: v (cout, cin, taps), w[co][ci][j] = v[co][ci][j] * scale[co]
//   transposed == u: v is a ConvTranspose1d weight (cin, cout / u, 2u), stride u, padding u / 2, run as a 3-tap convolution to
//                    u * Cout rows whose time-major output [L][u * Cout] IS the upsampled [L * u][Cout]:
//                    row r * Cout + co, tap dq + 1 = v[ci][co][r + u / 2 - u * dq] * scale[ci] where that tap index is in [0, 2u), else 0
hipError_t launch_ffg_pack_conv(int dtype, const float* v, const float* scale, int cout, int cin, int taps, int transposed, void* wfrag, hipStream_t s);
// dst[j][ci] = v[0][ci][j] * scale[0]: the fp32 weights of conv_post
hipError_t launch_ffg_pack_post(const float* v, const float* scale, int cin, int taps, float* dst, hipStream_t s);
// bias of the transposed conv's u * Cout rows: dst[r * Cout + co] = bias[co]
hipError_t launch_ffg_tile_bias(const float* bias, int cout, int u, float* dst, hipStream_t s);

// audio[item][t] = tanh(pre), pre = bias + sum_j sum_ci w[j][ci] * silu(x[t + j - taps/2][ci]), all fp32 (head.py:245-247); x: [items][L][C],
// C a multiple of 16, taps odd <= kFfgMaxTaps; pre (optional) receives the pre-tanh signal
hipError_t launch_ffg_post(const float* x, const float* w, const float* bias, int n_items, int L, int C, int taps, float* pre, float* audio, hipStream_t s);
// The same on packed rows: item b's utt[b].T * hop samples start at packed row utt[b].row0 * hop of x (and of pre); the audio stays padded,
// (n_items, L) with L = Tmax * hop, and audio[b][t] = 0 from utt[b].T * hop on (every sample is written)
hipError_t launch_ffg_post_ragged(const float* x, const float* w, const float* bias, const VocUtt* utt, int hop, int n_items, int L, int C, int taps,
                                  float* pre, float* audio, hipStream_t s);

}  // namespace st
