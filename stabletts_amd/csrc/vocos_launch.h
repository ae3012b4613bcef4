// Launcher interface of the Vocos vocoder kernels (vocos_kernels.hip); the GEMMs of the backbone and the head reuse
// the implicit-GEMM convolution kernels of launch.h.
// Reference: vocoders/vocos/models/backbone.py:50-56, module.py:33-46, head.py:39-72,93-117.
#pragma once
#include "launch.h"

namespace st {

// backbone widths the row kernels are built for: 64 lanes x 8, 12 or 16 channels (config.py:48 -> 512; vocoders/vocos/config.py:23 -> 768)
constexpr bool voc_dim_supported(int C) { return C == 512 || C == 768 || C == 1024; }
// ISTFT sizes of the inference path: n_fft in {256, 512, 1024, 2048} with hop_length == n_fft / 4 (every output sample sums at most
// four frames).  The training path (engine_vocos_train.cpp) keeps the preset alone: kVocNfft / kVocHop.
constexpr bool voc_nfft_supported(int n_fft) { return n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048; }
// channel pitch of the magnitude / phase planes in the head GEMM output: n_fft / 2 + 1 bins rounded up to the 128-column tile
constexpr int voc_head_plane(int n_fft) { return (n_fft / 2 + 1 + 127) / 128 * 128; }
// pitch of an im2col row: the embed GEMM walks K in 64-channel chunks, so the 7 * M columns are followed by zeros up to the next chunk
constexpr int voc_im2col_pitch(int M) { return (7 * M + 63) / 64 * 64; }
constexpr int kVocNfft = 2048;      // config.py:6
constexpr int kVocHop = 512;        // config.py:8
constexpr int kVocBins = kVocNfft / 2 + 1;
constexpr int kVocHeadPlane = voc_head_plane(kVocNfft);      // 1152 (1025 -> 9 x 128)

// A16[b*T + t][j*M + c] = mel[b][c][t + j - 3]  (0 outside [0, T)): the k = 7 embed convolution as one GEMM with K = 7*M.  Rows have
// the pitch voc_im2col_pitch(M); the columns from 7*M on are written as zero on every call (the workspace is reused, and a zero
// weight times a stale NaN is NaN)
hipError_t launch_voc_im2col7(int dtype, const float* mel, int B, int M, int T, void* a16, hipStream_t s);
// y = LayerNorm_C(x) * w + b  (eps 1e-6, C = 512, 768 or 1024; rows of C floats): out32 and/or out16 (may alias x for out32)
hipError_t launch_voc_ln(int dtype, const float* x, const float* w, const float* b, int64_t rows, int C, float* out32, void* out16,
                         void* out16_lo, hipStream_t s);      // out16_lo (optional): x - float(round16(x)), the low half of a split-precision operand
// h16 = LayerNorm_C(dwconv7(x) + bias) * w + b   per utterance (rows of different items never mix); dw: [C][7]
hipError_t launch_voc_dwconv_ln(int dtype, const float* x, const float* dw, const float* dbias, const float* w, const float* b,
                                int B, int T, int C, void* h16, hipStream_t s);
// head output rows [rows][2 * voc_head_plane(n_fft)] fp32 (log-magnitude plane, phase plane) -> windowed frames [rows][n_fft]
hipError_t launch_voc_spec_ifft(const float* head, const float* window, int64_t rows, int n_fft, float* frames, hipStream_t s);
// overlap-add with hop n_fft / 4, "same" trim, envelope normalisation: audio[b][T * n_fft / 4]
hipError_t launch_voc_overlap_add(const float* frames, const float* window, int B, int T, int n_fft, float* audio, hipStream_t s);

// ---- ragged batches: utterance b owns the packed rows row0 .. row0 + T of every row tensor (R = sum of T_b rows); the mel and
// the audio stay padded, (B, M, Tmax) and (B, Tmax * hop).  The host writes one VocUtt per utterance; launch_voc_segments
// expands them on the device into the block table of the im2col kernel and the wave table of the depthwise kernel.
struct VocUtt { int row0, T, tile0, grp0; };     // first packed row, frames, first 64-frame tile, first depthwise group
struct VocSeg { int row0, t0, T, item; };        // frames t0 .. of utterance `item`, whose T frames start at packed row row0
constexpr long long kVocMaxPaddedFrames = (1ll << 23) - 1;      // B * Tmax of one ragged overlap-add launch

int voc_dw_frames(int64_t rows);      // frames per wave of the depthwise kernel (4 from 8192 rows, else 1, at every width): the group length
// tiles: sum ceil(T_b / 64) entries, groups: sum ceil(T_b / dw_frames) entries
hipError_t launch_voc_segments(const VocUtt* utt, int B, int dw_frames, VocSeg* tiles, VocSeg* groups, hipStream_t s);
// launch_voc_im2col7 on frames 0 .. T_b - 1 of each utterance (taps outside are zero), into packed rows
hipError_t launch_voc_im2col7_ragged(int dtype, const float* mel, const VocSeg* tiles, int n_tiles, int M, int Tmax, void* a16, hipStream_t s);
// launch_voc_dwconv_ln on packed rows: a window never leaves its utterance; same arithmetic as the dense kernel
hipError_t launch_voc_dwconv_ln_ragged(int dtype, const float* x, const float* dw, const float* dbias, const float* w, const float* b,
                                       const VocSeg* groups, int n_groups, int dw_frames, int C, void* h16, hipStream_t s);
// launch_voc_overlap_add on packed frames; audio[b][s] = 0 for s >= T_b * hop (every sample of the padded audio is written)
hipError_t launch_voc_overlap_add_ragged(const float* frames, const float* window, const VocUtt* utt, int B, int Tmax, int n_fft, float* audio,
                                         hipStream_t s);

}  // namespace st
