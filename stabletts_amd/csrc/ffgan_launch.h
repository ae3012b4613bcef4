// Launcher interface of the FireflyGAN vocoder kernels (ffgan_kernels.hip): the row kernels of the ConvNeXt encoder at a
// run-time width (its GEMMs reuse the implicit-GEMM kernels of launch.h, as the Vocos engine does) and the convolution
// family of the HiFi-GAN head.  Reference: vocoders/ffgan/backbone.py:146-214, head.py:25-133,136-249 (use_template=False).
// Activations are time-major [item][L][C]; fp32 residual stream, 16-bit MFMA operands, fp32 accumulation.
// Split-precision mode (the "f16_split" / "bf16_split" handles): every MFMA operand x is the pair hi = fl16(x), lo = fl16(x - hi) and
// every product runs as w_hi x_hi + w_hi x_lo + w_lo x_hi (f16; bf16 needs more: see the encoder's and the head's notes below).  The launchers below that take `dtype` keep it as the
// 16-bit format; the split forms are siblings, so the default mode's kernels are the ones it had before.
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

// ---- split-precision producers of the encoder's GEMM operands.  Every one writes a PAIR tensor: row r = [hi (K values) | lo (K values)],
// hi = the 16-bit operand the default mode writes (bit for bit), lo = fl16(x - hi) of the same fp32 value x.  One pair tensor is one
// GEMM source a0 with c0 = 2 K; c2 = K re-reads its hi half (K = [hi | lo | hi] against [W_hi | W_hi | W_lo]: f16), c2 = 2 K both halves
// (K = [hi | lo | hi | lo] against [W_hi | W_hi | W_lo | W_lo]: bf16, whose lo * lo term is not negligible).
// launch_ffg_ln with the pair [rows][2 C] in place of out16
hipError_t launch_ffg_ln_split(int dtype, const float* x, const float* w, const float* b, int64_t rows, int C, float* out32, void* pair16, hipStream_t s);
// launch_ffg_dwconv_ln / _ragged (frames != nullptr: packed rows, B and T unused) with the pair [rows][2 C]
hipError_t launch_ffg_dwconv_ln_split(int dtype, const float* x, const float* dw, const float* dbias, const float* w, const float* b,
                                      int B, int T, const VocSeg* frames, int64_t rows, int C, void* pair16, hipStream_t s);
// the stem's im2col rows A[row][j * M + c] = mel[b][c][t + j - 3] (0 outside the utterance) as the pair [rows][2 * 7 M]; tiles == nullptr: the
// dense batch (B, M, T), else the 64-frame tile table of a ragged batch (vocos_launch.h: launch_voc_segments) over the padded mel (., M, T)
hipError_t launch_ffg_im2col7_split(int dtype, const float* mel, int B, int M, int T, const VocSeg* tiles, int n_tiles, void* a16, hipStream_t s);
// the pair [rows][2 F] of GELU(x) (exact erf form, nn.GELU()), x fp32 [rows][F]: pwconv1 runs as an fp32-output GEMM in split mode
hipError_t launch_ffg_gelu_split(int dtype, const float* x, int64_t rows, int F, void* u16, hipStream_t s);
// dst[co][part * K + j * cin + c], K = taps * cin, parts 0, 1 = fl16(w), parts 2 (and 3 of `parts` = 4) = fl16(w - fl16(w)), w = src[co][c][j]:
// the stem's weight (launch_pack_weight's column slices cannot express taps > 1 here: its K order is tap-major per slice)
hipError_t launch_ffg_pack_rows_split(int dtype, const float* src, int cout, int cin, int taps, int parts, void* dst, hipStream_t s);

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
    // Split mode (launch_ffg_conv_split) only: in32 is staged as it is, without the SiLU (conv_pre on the encoder's fp32 output)
    int in_raw;
};
// Split mode: the patch holds one plane per part of the operand, so a chunk is kFfgSplitKc channels.  f16: two parts (hi, lo) --
// 2 * 178 rows * (64 * 2 + 16) bytes = 51 264 at the largest halo, within the 64 KB a kernel gets without an opt-in.  bf16: THREE parts
// (hi, mid = fl16(x - hi), lo = fl16(x - hi - mid): 24 bits, the fp32 value itself) and six products -- a bf16 pair carries 16 bits, and
// through the head's ~40 sequential convs its rounding is the whole error of the waveform (1e-5); three planes are up to 76 896 bytes,
// which the launcher opts in to.  The fragment stream is [tile][chunk][k-step][part][lane][8].
constexpr int kFfgSplitKc = 64;
inline int ffg_split_planes(int dtype) { return dtype == DT_BF16 ? 3 : 2; }
// planes: 1 = the default mode, 2 / 3 = ffg_split_planes of a split handle
inline int ffg_kc(int cin, int planes = 1) { const int m = planes > 1 ? kFfgSplitKc : 128; return cin < m ? cin : m; }
inline int ffg_ksteps(int cin, int taps, int planes = 1) { const int kc = ffg_kc(cin, planes); return (cin / kc) * ((taps * kc + 31) / 32); }
inline size_t ffg_frag_bytes(int cout, int cin, int taps, int planes = 1) {
    return (size_t)(cout / 16) * ffg_ksteps(cin, taps, planes) * 1024 * planes;
}
// The fragment stream's index map, shared by the packing kernel and its host check (tests/host/ffgan_pack_index_check.cpp).  Element
// idx of the (hi) stream [tile][chunk][k-step][lane][8] is the MFMA A operand's W[co = 16 tile + (lane & 15)][k = 32 k-step + 8 (lane >> 4) + e]
// with k = tap * kc + (ci - chunk * kc).  -> the element's index into v, or -1 for a zero (the K padding; a polyphase tap outside
// [0, 2u)); *scale_row: its row of the weight-norm scale.  u == 0: v (cout, cin, taps); u > 0: the ConvTranspose1d weight
// (cin, cout / u, 2u) as the 3-tap convolution to u * Cout rows (launch_ffg_pack_conv).
__host__ __device__ inline long long ffg_frag_source(long long idx, int cout, int cin, int taps, int u, bool split, int* scale_row) {
    const int m = split ? kFfgSplitKc : 128, kc = cin < m ? cin : m, nchunks = cin / kc, ksc = (taps * kc + 31) >> 5;
    const int e = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
    long long rest = idx >> 9;
    const int ks = (int)(rest % ksc); rest /= ksc;
    const int ch = (int)(rest % nchunks);
    const int tile = (int)(rest / nchunks);
    const int co = tile * 16 + (lane & 15), kk = ks * 32 + 8 * (lane >> 4) + e;
    const int tap = kk / kc, ci = ch * kc + kk % kc;
    if (tap >= taps) return -1;
    if (u == 0) { *scale_row = co; return ((long long)co * cin + ci) * taps + tap; }
    const int Co = cout / u, r = co / Co, c = co - r * Co;
    const int j = r + u / 2 - u * (tap - 1);
    if (j < 0 || j >= 2 * u) return -1;
    *scale_row = ci;
    return ((long long)ci * Co + c) * (2 * u) + j;
}
// where element idx of the hi stream lands in the 16-bit buffer: itself (planes = 1), or part `plane` of its k-step's `planes` fragments
__host__ __device__ inline long long ffg_frag_offset(long long idx, int planes, int plane) {
    return planes > 1 ? (idx >> 9) * 512 * planes + plane * 512 + (idx & 511) : idx;
}
// cin: 16, 32, 64 or a multiple of 128; cout a multiple of 16; taps odd <= kFfgMaxTaps; halo <= kFfgMaxHalo
bool ffg_conv_supported(int cin, int cout, int taps, int dil);
hipError_t launch_ffg_conv(int dtype, const FfgConvArgs& a, hipStream_t s);
// The same family with SPLIT operands: in32 only (SiLU while staging unless in_raw; the staged value is split into the two planes),
// FFG_F32 or FFG_RES, wfrag from launch_ffg_pack_conv(..., split = true).  f16: three MFMAs per (frame, channel) fragment pair,
// w_hi b_hi + w_hi b_lo + w_lo b_hi; bf16: six, w_hi b_hi + w_hi b_mid + w_mid b_hi + w_mid b_mid + w_hi b_lo + w_lo b_hi (every product
// down to 2^-24 of the largest); in that order into one fp32 accumulator.  Dense, ragged and the bitwise guarantees as above.
hipError_t launch_ffg_conv_split(int dtype, const FfgConvArgs& a, hipStream_t s);

// scale[r] = g[r] / ||v[r, :]||_2 over the `inner` elements of row r (weight norm over all dims but 0)
hipError_t launch_ffg_wn_scale(const float* v, const float* g, int rows, int inner, float* scale, hipStream_t s);
// Fragment-ordered 16-bit weights of one convolution from the weight-norm direction v and scale (scale == nullptr: v is the weight).
//   transposed == 0: v (cout, cin, taps), w[co][ci][j] = v[co][ci][j] * scale[co]
//   transposed == u: v is a ConvTranspose1d weight (cin, cout / u, 2u), stride u, padding u / 2, run as a 3-tap convolution to
//                    u * Cout rows whose time-major output [L][u * Cout] IS the upsampled [L * u][Cout]:
//                    row r * Cout + co, tap dq + 1 = v[ci][co][r + u / 2 - u * dq] * scale[ci] where that tap index is in [0, 2u), else 0
// split: the stream of launch_ffg_conv_split -- chunks of kFfgSplitKc channels, every k-step's hi fragment followed by its lo fragment
//        (bf16: mid, then lo), lo = fl16(w - fl16(w)) of the folded, scaled weight w (an fp32 value: the product is rounded to fp32
//        before it is split)
hipError_t launch_ffg_pack_conv(int dtype, const float* v, const float* scale, int cout, int cin, int taps, int transposed, void* wfrag, hipStream_t s,
                                bool split = false);
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
