// Vocos vocoder: the kernels around its GEMMs (vocoders/vocos/models/*.py; config.py:46-50 -> 128 -> 512, 8 ConvNeXt
// blocks, ISTFT head n_fft 2048 / hop 512; the Vocos trainer's vocoders/vocos/config.py:21-26 -> 128 -> 768, 12 blocks).  Everything here is row-wise HBM-bound work on time-major tensors
// [utterance][frame][channel]; the five GEMM shapes run on the implicit-GEMM kernels of conv_gemm2_impl.h.
#include "audio_fft.h"
#include "common.h"
#include "vocos_launch.h"

#include <type_traits>

namespace st {

// ---------------------------------------------------------------- embed: im2col of the k = 7 convolution (backbone.py:28,51)
// One block = 64 frames of one utterance: the (M x 70) mel tile is read with frames contiguous and written as
// 16-bit rows [frame][tap][channel] of pitch voc_im2col_pitch(M).  src: the utterance's mel (M, ld), T <= ld of its frames valid; rows: its frame 0.
template <class P>
__device__ __forceinline__ void voc_im2col7_tile(const float* __restrict__ src, int M, int ld, int T, int t0,
                                                 typename P::elem* __restrict__ rows, float* tile /* [M][72] */) {
    for (int i = threadIdx.x; i < M * 70; i += 256) {
        const int c = i / 70, k = i - c * 70;
        const int t = t0 + k - 3;
        tile[c * 72 + k] = (t >= 0 && t < T) ? src[(size_t)c * ld + t] : 0.0f;
    }
    __syncthreads();
    const int K = 7 * M, Kp = voc_im2col_pitch(M);      // columns K .. Kp - 1: the zero tail of the last 64-channel chunk
    for (int i = threadIdx.x; i < 64 * Kp; i += 256) {
        const int f = i / Kp, r = i - f * Kp;
        const int j = r / M, c = r - j * M;
        if (t0 + f < T) rows[((size_t)t0 + f) * Kp + r] = to16<P>(r < K ? tile[c * 72 + f + j] : 0.0f);
    }
}

template <class P>
__global__ __launch_bounds__(256) void voc_im2col7_kernel(const float* __restrict__ mel, int M, int T, typename P::elem* __restrict__ a16) {
    extern __shared__ float tile[];           // [M][72]
    const int b = blockIdx.y;
    voc_im2col7_tile<P>(mel + (size_t)b * M * T, M, T, T, blockIdx.x * 64, a16 + (size_t)b * T * voc_im2col_pitch(M), tile);
}

// Ragged batch: block = one entry of the tile table (voc_segments_kernel); mel is padded (B, M, Tmax), the rows are packed.
template <class P>
__global__ __launch_bounds__(256) void voc_im2col7_ragged_kernel(const float* __restrict__ mel, const VocSeg* __restrict__ tiles, int M, int Tmax,
                                                                 typename P::elem* __restrict__ a16) {
    extern __shared__ float tile[];           // [M][72]
    const VocSeg sg = tiles[blockIdx.x];
    voc_im2col7_tile<P>(mel + (size_t)sg.item * M * Tmax, M, Tmax, sg.T, sg.t0, a16 + (size_t)sg.row0 * voc_im2col_pitch(M), tile);
}

hipError_t launch_voc_im2col7(int dtype, const float* mel, int B, int M, int T, void* a16, hipStream_t s) {
    const dim3 grid((T + 63) / 64, B), blk(256);
    const size_t lds = (size_t)M * 72 * 4;
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    if (dtype == DT_BF16) hipLaunchKernelGGL((voc_im2col7_kernel<OpBF16>), grid, blk, lds, s, mel, M, T, (OpBF16::elem*)a16);
    else                  hipLaunchKernelGGL((voc_im2col7_kernel<OpF16>), grid, blk, lds, s, mel, M, T, (OpF16::elem*)a16);
    return hipGetLastError();
}

hipError_t launch_voc_im2col7_ragged(int dtype, const float* mel, const VocSeg* tiles, int n_tiles, int M, int Tmax, void* a16, hipStream_t s) {
    const dim3 grid(n_tiles), blk(256);
    const size_t lds = (size_t)M * 72 * 4;
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    if (dtype == DT_BF16) hipLaunchKernelGGL((voc_im2col7_ragged_kernel<OpBF16>), grid, blk, lds, s, mel, tiles, M, Tmax, (OpBF16::elem*)a16);
    else                  hipLaunchKernelGGL((voc_im2col7_ragged_kernel<OpF16>), grid, blk, lds, s, mel, tiles, M, Tmax, (OpF16::elem*)a16);
    return hipGetLastError();
}

// ---------------------------------------------------------------- ragged batches: the tables of the three kernels that know utterances
// One block per utterance expands its VocUtt (host table) into the 64-frame tiles of the im2col kernel and the dw_frames-frame
// groups of the depthwise kernel: a block / wave of those kernels reads one entry and never searches.
__global__ __launch_bounds__(256) void voc_segments_kernel(const VocUtt* __restrict__ utt, int dw_frames, VocSeg* __restrict__ tiles,
                                                           VocSeg* __restrict__ groups) {
    const int b = blockIdx.x;
    const VocUtt u = utt[b];
    for (int i = threadIdx.x; i * 64 < u.T; i += 256) tiles[u.tile0 + i] = VocSeg{u.row0, i * 64, u.T, b};
    for (int i = threadIdx.x; (long long)i * dw_frames < u.T; i += 256) groups[u.grp0 + i] = VocSeg{u.row0, i * dw_frames, u.T, b};
}

hipError_t launch_voc_segments(const VocUtt* utt, int B, int dw_frames, VocSeg* tiles, VocSeg* groups, hipStream_t s) {
    hipLaunchKernelGGL(voc_segments_kernel, dim3(B), dim3(256), 0, s, utt, dw_frames, tiles, groups);
    return hipGetLastError();
}

// ---------------------------------------------------------------- row kernels: LayerNorm and depthwise conv + LayerNorm, one wave per row
// A row of C = 64 * CPL channels (CPL = 8, 12, 16 channels per lane: dim 512, 768, 1024) lives in one wave as CPL / 4 float4 per lane.
// Channel mapping.  CPL = 8 (dim 512) keeps the mapping it was written with: a contiguous run, lane = channels 8 lane .. 8 lane + 7,
// one 16-byte store of its 8 16-bit outputs.  CPL = 12 and 16 take float4 j of a lane at channel (j * 64 + lane) * 4 instead: every
// load of the wave is then one contiguous 1 KiB segment and every 16-bit store one contiguous 512 B segment, where a contiguous run of
// 12 channels would make the lane's 24-byte output straddle 16-byte alignment and spread each load instruction over three times its
// bytes.  The GEMM operand is row-major [row][C] either way, and the statistics are sums over the whole row.
template <int CPL> struct VocRow { float v[CPL]; };

// the lane's first channel, and the channel distance between its float4s: float4 j sits at voc_ch0 + j * voc_qs
template <int CPL> __device__ __forceinline__ int voc_ch0(int lane) { return CPL == 8 ? lane * 8 : lane * 4; }
template <int CPL> constexpr int voc_qs() { return CPL == 8 ? 4 : 256; }
// channel of element i of a lane's VocRow, relative to voc_ch0
template <int CPL> constexpr int voc_rel(int i) { return (i / 4) * voc_qs<CPL>() + (i & 3); }

template <int CPL>
__device__ __forceinline__ VocRow<CPL> voc_ld(const float* p /* the lane's first channel of the row */) {
    VocRow<CPL> r;
#pragma unroll
    for (int j = 0; j < CPL / 4; ++j) {
        const float4 q = *(const float4*)(p + j * voc_qs<CPL>());
        r.v[4 * j] = q.x; r.v[4 * j + 1] = q.y; r.v[4 * j + 2] = q.z; r.v[4 * j + 3] = q.w;
    }
    return r;
}

// LayerNorm(C, eps 1e-6, affine) of the wave's row: mean and biased variance by two wave reductions
template <int CPL>
__device__ __forceinline__ void voc_ln_row(VocRow<CPL>& r, const VocRow<CPL>& w, const VocRow<CPL>& b) {
    constexpr float inv_c = 1.0f / (64.0f * CPL);
    float sum = r.v[0];
#pragma unroll
    for (int i = 1; i < CPL; ++i) sum = sum + r.v[i];
    const float mean = wave_sum(sum) * inv_c;
#pragma unroll
    for (int i = 0; i < CPL; ++i) r.v[i] -= mean;
    float sq = r.v[0] * r.v[0];
#pragma unroll
    for (int i = 1; i < CPL; ++i) sq = sq + r.v[i] * r.v[i];
    const float var = wave_sum(sq) * inv_c;
    const float rs = 1.0f / sqrtf(var + 1e-6f);
#pragma unroll
    for (int i = 0; i < CPL; ++i) r.v[i] = r.v[i] * rs * w.v[i] + b.v[i];
}

template <int CPL>
__device__ __forceinline__ void voc_st32(float* p /* the lane's first channel of the row */, const VocRow<CPL>& r) {
#pragma unroll
    for (int j = 0; j < CPL / 4; ++j) *(float4*)(p + j * voc_qs<CPL>()) = make_float4(r.v[4 * j], r.v[4 * j + 1], r.v[4 * j + 2], r.v[4 * j + 3]);
}

template <class P, int CPL>
__device__ __forceinline__ void voc_st16(void* p /* the lane's first channel of the 16-bit row */, const VocRow<CPL>& r) {
    if (CPL == 8) {
        const uint2 lo = pack4<P>(r.v[0], r.v[1], r.v[2], r.v[3]), hi = pack4<P>(r.v[4], r.v[5], r.v[6], r.v[7]);
        *(uint4*)p = make_uint4(lo.x, lo.y, hi.x, hi.y);
    } else {
#pragma unroll
        for (int j = 0; j < CPL / 4; ++j)
            *(uint2*)((unsigned char*)p + j * voc_qs<CPL>() * 2) = pack4<P>(r.v[4 * j], r.v[4 * j + 1], r.v[4 * j + 2], r.v[4 * j + 3]);
    }
}

template <class P, int CPL>
__global__ __launch_bounds__(256) void voc_ln_kernel(const float* x, const float* __restrict__ w, const float* __restrict__ b,
                                                     long long rows, float* out32, void* out16, void* out16_lo) {
    constexpr int C = 64 * CPL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int ch = voc_ch0<CPL>(lane);
    VocRow<CPL> v = voc_ld<CPL>(x + (size_t)row * C + ch);
    voc_ln_row<CPL>(v, voc_ld<CPL>(w + ch), voc_ld<CPL>(b + ch));
    if (out32) voc_st32<CPL>(out32 + (size_t)row * C + ch, v);
    if (out16) voc_st16<P, CPL>((unsigned char*)out16 + ((size_t)row * C + ch) * 2, v);
    if (out16_lo) {      // the low half of a split-precision operand pair: x - float(round16(x)), rounded once more
        VocRow<CPL> r;
#pragma unroll
        for (int i = 0; i < CPL; ++i) r.v[i] = v.v[i] - (float)to16<P>(v.v[i]);
        voc_st16<P, CPL>((unsigned char*)out16_lo + ((size_t)row * C + ch) * 2, r);
    }
}

// C -> f(channels per lane) on the instantiation that runs it (st_create_vocoder admits no other width)
template <class F>
static hipError_t voc_for_cpl(int C, F&& f) {
    switch (C) {
        case 512:  f(std::integral_constant<int, 8>()); break;
        case 768:  f(std::integral_constant<int, 12>()); break;
        case 1024: f(std::integral_constant<int, 16>()); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_voc_ln(int dtype, const float* x, const float* w, const float* b, int64_t rows, int C, float* out32, void* out16,
                         void* out16_lo, hipStream_t s) {
    const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
    return voc_for_cpl(C, [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        if (dtype == DT_BF16) hipLaunchKernelGGL((voc_ln_kernel<OpBF16, CPL>), grid, blk, 0, s, x, w, b, (long long)rows, out32, out16, out16_lo);
        else                  hipLaunchKernelGGL((voc_ln_kernel<OpF16, CPL>), grid, blk, 0, s, x, w, b, (long long)rows, out32, out16, out16_lo);
    });
}

// ---------------------------------------------------------------- ConvNeXt block prologue: depthwise k = 7 conv + LayerNorm (module.py:35-37)
// One wave per R consecutive frames of one utterance (R = 4; 1 for small batches), lane = CPL channels: the R + 6 fp32 residual
// rows of the window are requested up front and the 7 * CPL taps of the lane's channels loaded once per wave.  Live values per lane:
// (R + 6) * CPL window + 7 * CPL taps + 3 * CPL bias / LayerNorm affine + CPL accumulators -- at R = 4 168 for CPL = 8, 252 for 12 and
// 336 for 16, which the unified register file of one wave per SIMD (launch bound 256 threads: 512 registers) holds without scratch.
template <class P, int CPL, int R>
__device__ __forceinline__ void voc_dwconv_ln_group(const float* __restrict__ xi /* the utterance's frame 0, + ch */, int T, int t0,
                                                    const float* __restrict__ dw, const float* __restrict__ dbias,
                                                    const float* __restrict__ w, const float* __restrict__ b, int ch,
                                                    unsigned char* hi /* h16 of the utterance's frame 0, + ch */) {
    constexpr int C = 64 * CPL;
    VocRow<CPL> zero;
#pragma unroll
    for (int i = 0; i < CPL; ++i) zero.v[i] = 0.0f;
    VocRow<CPL> win[R + 6];   // every row of the window is requested before anything is computed: one exposed latency per wave
#pragma unroll
    for (int j = 0; j < R + 6; ++j) {
        const int t = t0 - 3 + j;
        win[j] = (t >= 0 && t < T) ? voc_ld<CPL>(xi + (size_t)t * C) : zero;      // zero padding of nn.Conv1d(padding=3)
    }
    float wt[CPL][7];
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) wt[i][j] = dw[(size_t)(ch + voc_rel<CPL>(i)) * 7 + j];
    const VocRow<CPL> bias = voc_ld<CPL>(dbias + ch), lw = voc_ld<CPL>(w + ch), lb = voc_ld<CPL>(b + ch);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int t = t0 + r;
        if (t >= T) break;                          // wave-uniform
        VocRow<CPL> acc = bias;
#pragma unroll
        for (int j = 0; j < 7; ++j)
#pragma unroll
            for (int i = 0; i < CPL; ++i) acc.v[i] += wt[i][j] * win[r + j].v[i];
        voc_ln_row<CPL>(acc, lw, lb);
        voc_st16<P, CPL>(hi + (size_t)t * C * 2, acc);
    }
}

template <class P, int CPL, int R>
__global__ __launch_bounds__(256) void voc_dwconv_ln_kernel(const float* __restrict__ x, const float* __restrict__ dw,
                                                            const float* __restrict__ dbias, const float* __restrict__ w,
                                                            const float* __restrict__ b, int T, int groups_per_item, long long n_groups,
                                                            void* h16) {
    constexpr int C = 64 * CPL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long grp = (long long)blockIdx.x * 4 + wave;
    if (grp >= n_groups) return;
    const int item = (int)(grp / groups_per_item);
    const int t0 = (int)(grp - (long long)item * groups_per_item) * R;
    const int ch = voc_ch0<CPL>(lane);
    voc_dwconv_ln_group<P, CPL, R>(x + (size_t)item * T * C + ch, T, t0, dw, dbias, w, b, ch,
                                   (unsigned char*)h16 + ((size_t)item * T * C + ch) * 2);
}

// Ragged batch: wave = one entry of the group table (R frames of ONE utterance, voc_segments_kernel), read through scalar
// registers; x and h16 are packed rows.
template <class P, int CPL, int R>
__global__ __launch_bounds__(256) void voc_dwconv_ln_ragged_kernel(const float* __restrict__ x, const float* __restrict__ dw,
                                                                   const float* __restrict__ dbias, const float* __restrict__ w,
                                                                   const float* __restrict__ b, const VocSeg* __restrict__ groups,
                                                                   int n_groups, void* h16) {
    constexpr int C = 64 * CPL;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long grp = (long long)blockIdx.x * 4 + wave;
    if (grp >= n_groups) return;
    const VocSeg sg = groups[grp];
    const int ch = voc_ch0<CPL>(lane);
    voc_dwconv_ln_group<P, CPL, R>(x + (size_t)sg.row0 * C + ch, sg.T, sg.t0, dw, dbias, w, b, ch,
                                   (unsigned char*)h16 + ((size_t)sg.row0 * C + ch) * 2);
}

template <class P, int CPL, int R>
static void launch_dw(const float* x, const float* dw, const float* dbias, const float* w, const float* b, int B, int T, void* h16, hipStream_t s) {
    const int gpi = (T + R - 1) / R;
    const long long n_groups = (long long)B * gpi;
    hipLaunchKernelGGL((voc_dwconv_ln_kernel<P, CPL, R>), dim3((unsigned)((n_groups + 3) / 4)), dim3(256), 0, s, x, dw, dbias, w, b, T, gpi, n_groups, h16);
}

hipError_t launch_voc_dwconv_ln(int dtype, const float* x, const float* dw, const float* dbias, const float* w, const float* b,
                                int B, int T, int C, void* h16, hipStream_t s) {
    const bool big = voc_dw_frames((int64_t)B * T) == 4;      // small batches: one frame per wave (more waves than a few CUs' worth)
    return voc_for_cpl(C, [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        if (dtype == DT_BF16) { if (big) launch_dw<OpBF16, CPL, 4>(x, dw, dbias, w, b, B, T, h16, s); else launch_dw<OpBF16, CPL, 1>(x, dw, dbias, w, b, B, T, h16, s); }
        else                  { if (big) launch_dw<OpF16, CPL, 4>(x, dw, dbias, w, b, B, T, h16, s); else launch_dw<OpF16, CPL, 1>(x, dw, dbias, w, b, B, T, h16, s); }
    });
}

template <class P, int CPL, int R>
static void launch_dw_ragged(const float* x, const float* dw, const float* dbias, const float* w, const float* b, const VocSeg* groups,
                             int n_groups, void* h16, hipStream_t s) {
    hipLaunchKernelGGL((voc_dwconv_ln_ragged_kernel<P, CPL, R>), dim3((unsigned)(((long long)n_groups + 3) / 4)), dim3(256), 0, s, x, dw, dbias, w, b,
                       groups, n_groups, h16);
}

int voc_dw_frames(int64_t rows) { return rows >= 8192 ? 4 : 1; }

hipError_t launch_voc_dwconv_ln_ragged(int dtype, const float* x, const float* dw, const float* dbias, const float* w, const float* b,
                                       const VocSeg* groups, int n_groups, int dw_frames, int C, void* h16, hipStream_t s) {
    const bool big = dw_frames == 4;
    return voc_for_cpl(C, [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        if (dtype == DT_BF16) { if (big) launch_dw_ragged<OpBF16, CPL, 4>(x, dw, dbias, w, b, groups, n_groups, h16, s); else launch_dw_ragged<OpBF16, CPL, 1>(x, dw, dbias, w, b, groups, n_groups, h16, s); }
        else                  { if (big) launch_dw_ragged<OpF16, CPL, 4>(x, dw, dbias, w, b, groups, n_groups, h16, s); else launch_dw_ragged<OpF16, CPL, 1>(x, dw, dbias, w, b, groups, n_groups, h16, s); }
    });
}

// ---------------------------------------------------------------- ISTFT head (head.py:103-116, ISTFT.forward :50-57)
// One block (256 threads) per frame.  S[k] = min(exp(m_k), 100) (cos p_k + i sin p_k), k = 0..1024, then the real
// inverse FFT of length 2048 as ONE complex inverse FFT of length 1024:
//     E[k] = (S[k] + conj(S[1024-k])) / 2,   O[k] = (S[k] - conj(S[1024-k])) / 2 * e^{+2 pi i k / 2048},   Z = E + i O,
//     z = IDFT_1024(Z):   x[2n] = Re z[n],  x[2n+1] = Im z[n]
// (imaginary parts of the DC and Nyquist bins ignored, as a complex-to-real transform does).  The 1024-point
// transform is 5 radix-4 Stockham autosort passes between two LDS buffers; twiddles from an LDS table built per block.
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

__global__ __launch_bounds__(256) void voc_spec_ifft_kernel(const float* __restrict__ head, const float* __restrict__ window,
                                                            float* __restrict__ frames) {
    __shared__ float2 bufA[1024 + 8], bufB[1024 + 8], tw[1024];
    const int tid = threadIdx.x;
    const float* row = head + (size_t)blockIdx.x * (2 * kVocHeadPlane);
    for (int k = tid; k <= 1024; k += 256) {
        const float mag = fminf(expf(row[k]), 100.0f);           // head.py:105-106
        float sn, cs;
        sincosf(row[kVocHeadPlane + k], &sn, &cs);               // :108-109
        bufB[k] = make_float2(mag * cs, (k == 0 || k == 1024) ? 0.0f : mag * sn);
    }
    for (int k = tid; k < 1024; k += 256) {
        float sn, cs;
        sincospif((float)k * (1.0f / 512.0f), &sn, &cs);         // e^{+2 pi i k / 1024}
        tw[k] = make_float2(cs, sn);
    }
    __syncthreads();
    for (int k = tid; k < 1024; k += 256) {
        const float2 a = bufB[k], c = bufB[1024 - k];
        const float2 E = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));
        float2 O = make_float2(0.5f * (a.x - c.x), 0.5f * (a.y + c.y));
        float sn, cs;
        sincospif((float)k * (1.0f / 1024.0f), &sn, &cs);        // e^{+2 pi i k / 2048}
        O = cmul(O, make_float2(cs, sn));
        bufA[k] = make_float2(E.x - O.y, E.y + O.x);             // E + i O
    }
    __syncthreads();
    float2* in = bufA; float2* out = bufB;
#pragma unroll 1
    for (int Ns = 1; Ns < 1024; Ns <<= 2) {
        const int j = tid, k = j & (Ns - 1);
        const int tstep = k * (256 / Ns);                         // twiddle exponent of t = 1: k / (4 Ns) turns = k * 256 / Ns / 1024
        const float2 u0 = in[j];
        const float2 u1 = cmul(in[j + 256], tw[tstep]);
        const float2 u2 = cmul(in[j + 512], tw[2 * tstep]);
        const float2 u3 = cmul(in[j + 768], tw[3 * tstep]);
        const float2 s02 = make_float2(u0.x + u2.x, u0.y + u2.y), d02 = make_float2(u0.x - u2.x, u0.y - u2.y);
        const float2 s13 = make_float2(u1.x + u3.x, u1.y + u3.y), d13 = make_float2(u1.x - u3.x, u1.y - u3.y);
        const int j0 = ((j - k) << 2) + k;
        out[j0] = make_float2(s02.x + s13.x, s02.y + s13.y);
        out[j0 + Ns] = make_float2(d02.x - d13.y, d02.y + d13.x);       // u0 + i u1 - u2 - i u3
        out[j0 + 2 * Ns] = make_float2(s02.x - s13.x, s02.y - s13.y);
        out[j0 + 3 * Ns] = make_float2(d02.x + d13.y, d02.y - d13.x);   // u0 - i u1 - u2 + i u3
        __syncthreads();
        float2* tmp = in; in = out; out = tmp;
    }
    float* dst = frames + (size_t)blockIdx.x * kVocNfft;
    for (int n = tid; n < 1024; n += 256) {
        const float2 z = in[n];
        const float2 wv = *(const float2*)(window + 2 * n);
        *(float2*)(dst + 2 * n) = make_float2(z.x * (1.0f / 1024.0f) * wv.x, z.y * (1.0f / 1024.0f) * wv.y);   // :56-57
    }
}

// n_fft 256, 512, 1024: the same steps with S = 2048 / N frames per block, so that every thread still does one radix-4 butterfly per
// pass -- the H = N / 2 point Stockham transform of the feature front end (audio_fft.h: mel_fft<N>, with its radix-2 pass for H = 512
// and 128; mel_twiddles<N> holds e^{-2 pi i m / N}).  mel_fft is the forward transform, so the block transforms conj Z and conjugates
// the result, as mel_inverse_to_ws does: IDFT_H(Z) = conj(DFT_H(conj Z)).  The block of frames t0 .. t0 + S - 1 may reach past
// `rows`: a dead frame reads no head row (its spectrum is zero) and writes no frame.
template <int N>
__global__ __launch_bounds__(256) void voc_spec_ifft_small_kernel(const float* __restrict__ head, const float* __restrict__ window,
                                                                  long long rows, float* __restrict__ frames) {
    constexpr int H = MelGeo<N>::H, S = MelGeo<N>::S, plane = voc_head_plane(N);
    static_assert(S * H == 1024 && S * (H / 4) == 256, "one radix-4 butterfly per thread and pass");
    __shared__ float2 b0[S * H], b1[S * (H + 1)], tw[H];
    float2* spec = b1;      // the S spectra of H + 1 bins: read for the last time before mel_fft's first pass writes b1
    const int tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * S;
    mel_twiddles<N>(tw, tid);
    for (int e = tid; e < S * (H + 1); e += 256) {
        const int f = e / (H + 1), k = e - f * (H + 1);
        float2 v = make_float2(0.0f, 0.0f);
        if (t0 + f < rows) {
            const float* row = head + (size_t)(t0 + f) * (2 * plane);
            const float mag = fminf(expf(row[k]), 100.0f);           // head.py:105-106
            float sn, cs;
            sincosf(row[plane + k], &sn, &cs);                       // :108-109
            v = make_float2(mag * cs, (k == 0 || k == H) ? 0.0f : mag * sn);
        }
        spec[e] = v;
    }
    __syncthreads();
    for (int e = tid; e < S * H; e += 256) {
        const int f = e / H, k = e - f * H;
        const float2 a = spec[f * (H + 1) + k], c = spec[f * (H + 1) + H - k];
        const float2 E = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));
        float2 O = make_float2(0.5f * (a.x - c.x), 0.5f * (a.y + c.y));
        O = cmul(O, make_float2(tw[k].x, -tw[k].y));                 // e^{+2 pi i k / N}
        b0[e] = make_float2(E.x - O.y, -(E.y + O.x));                // conj(E + i O)
    }
    __syncthreads();
    const float2* zz = mel_fft<N>(b0, b1, tw, tid);                  // conj z: x[2n] = Re, x[2n+1] = -Im
    for (int e = tid; e < S * H; e += 256) {
        const int f = e / H, n = e - f * H;
        if (t0 + f >= rows) continue;
        const float2 z = zz[e];
        const float2 wv = *(const float2*)(window + 2 * n);
        *(float2*)(frames + (size_t)(t0 + f) * N + 2 * n) = make_float2(z.x * (1.0f / H) * wv.x, -z.y * (1.0f / H) * wv.y);   // :56-57
    }
}

// n_fft -> f(integral_constant<int, n_fft>) for the sizes st_create_vocoder admits
template <class F>
static hipError_t voc_for_nfft(int n_fft, F&& f) {
    switch (n_fft) {
        case 256:  f(std::integral_constant<int, 256>()); break;
        case 512:  f(std::integral_constant<int, 512>()); break;
        case 1024: f(std::integral_constant<int, 1024>()); break;
        case 2048: f(std::integral_constant<int, 2048>()); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_voc_spec_ifft(const float* head, const float* window, int64_t rows, int n_fft, float* frames, hipStream_t s) {
    return voc_for_nfft(n_fft, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        if constexpr (N == kVocNfft) {
            hipLaunchKernelGGL(voc_spec_ifft_kernel, dim3((unsigned)rows), dim3(256), 0, s, head, window, frames);
        } else {
            constexpr int S = MelGeo<N>::S;
            hipLaunchKernelGGL((voc_spec_ifft_small_kernel<N>), dim3((unsigned)((rows + S - 1) / S)), dim3(256), 0, s, head, window, (long long)rows, frames);
        }
    });
}

// Overlap-add (fold, head.py:60-63), "same" trim (:48,63), window envelope (:66-69) and normalisation (:73), hop = N / 4.
// Output sample s of utterance b sits at q = s + (N - hop) / 2 of the untrimmed signal (768 at N = 2048); frames
// floor((q - (N - 1) + hop - 1) / hop) .. floor(q / hop) cover it (at most 4), added in ascending frame order.
template <int N>
__device__ __forceinline__ float voc_ola_sample(const float* __restrict__ fr /* the utterance's frames */, const float* __restrict__ window,
                                                int T, long long s) {
    constexpr int hop = N / 4;
    const long long q = s + (N - hop) / 2;
    int f1 = (int)(q / hop); if (f1 > T - 1) f1 = T - 1;
    long long f0l = (q - (N - 1) + hop - 1) / hop; if (q - (N - 1) < 0) f0l = 0;
    float y = 0.0f, env = 0.0f;
    for (int f = (int)f0l; f <= f1; ++f) {
        const int off = (int)(q - (long long)f * hop);
        const float wv = window[off];
        y += fr[(size_t)f * N + off];
        env += wv * wv;
    }
    return y / env;
}

template <int N>
__global__ __launch_bounds__(256) void voc_overlap_add_kernel(const float* __restrict__ frames, const float* __restrict__ window,
                                                              int T, float* __restrict__ audio) {
    const long long len = (long long)T * (N / 4);
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= len) return;
    const int b = blockIdx.y;
    audio[(size_t)b * len + s] = voc_ola_sample<N>(frames + (size_t)b * T * N, window, T, s);
}

// Ragged batch: packed frames -> padded audio (B, Tmax * hop); `per` = ceil(Tmax * hop / 256) blocks per utterance on a 1-D grid,
// zeros from sample T_b * hop on.  With hop 64 or 128 the last block of an utterance can reach past Tmax * hop: those threads
// write nothing (the samples there are the next utterance's).
template <int N>
__global__ __launch_bounds__(256) void voc_overlap_add_ragged_kernel(const float* __restrict__ frames, const float* __restrict__ window,
                                                                     const VocUtt* __restrict__ utt, int Tmax, int per, float* __restrict__ audio) {
    constexpr int hop = N / 4;
    const int b = blockIdx.x / per;
    const long long s = (long long)(blockIdx.x - b * per) * 256 + threadIdx.x;
    if (s >= (long long)Tmax * hop) return;
    const VocUtt u = utt[b];
    audio[(size_t)b * Tmax * hop + s] = s < (long long)u.T * hop ? voc_ola_sample<N>(frames + (size_t)u.row0 * N, window, u.T, s) : 0.0f;
}

hipError_t launch_voc_overlap_add(const float* frames, const float* window, int B, int T, int n_fft, float* audio, hipStream_t s) {
    return voc_for_nfft(n_fft, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        const long long len = (long long)T * (N / 4);
        hipLaunchKernelGGL((voc_overlap_add_kernel<N>), dim3((unsigned)((len + 255) / 256), B), dim3(256), 0, s, frames, window, T, audio);
    });
}

hipError_t launch_voc_overlap_add_ragged(const float* frames, const float* window, const VocUtt* utt, int B, int Tmax, int n_fft, float* audio,
                                         hipStream_t s) {
    if ((long long)B * Tmax > kVocMaxPaddedFrames) return hipErrorInvalidValue;      // grid.x * 256 threads stays below 2^32 (per <= 2 * Tmax)
    return voc_for_nfft(n_fft, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        const int per = (int)(((long long)Tmax * (N / 4) + 255) / 256);
        hipLaunchKernelGGL((voc_overlap_add_ragged_kernel<N>), dim3((unsigned)((long long)B * per)), dim3(256), 0, s, frames, window, utt, Tmax, per, audio);
    });
}

}  // namespace st
