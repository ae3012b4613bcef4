// FireflyGAN vocoder (vocoders/ffgan): the row kernels of the ConvNeXt encoder at a run-time width and the kernels of the
// HiFi-GAN head -- one implicit-GEMM convolution family on the 16x16x32 MFMA (conv_pre, the 90 ResBlock convs, the five
// transposed convs as 3-tap convs with a pixel-shuffle store that the time-major layout makes a plain store), the weight-norm
// fold and fragment packing of st_finalize, and the fp32 SiLU -> conv_post -> tanh vector kernel.
#include "common.h"
#include "ffgan_launch.h"

#include <atomic>
#include <type_traits>

namespace st {

// ---------------------------------------------------------------- LayerNorm(C, eps 1e-6, affine): one wave per frame, lane = 2 channels of every 128
constexpr int kFfgNi = kFfgMaxDim / 128;

__device__ __forceinline__ void ffg_ln_rows(float2 (&v)[kFfgNi], int ni, int C) {      // v -> (v - mean) * rstd
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < kFfgNi; ++i) if (i < ni) sum += v[i].x + v[i].y;
    const float mean = wave_sum(sum) / (float)C;
    float sq = 0.0f;
#pragma unroll
    for (int i = 0; i < kFfgNi; ++i) if (i < ni) { v[i].x -= mean; v[i].y -= mean; sq += v[i].x * v[i].x + v[i].y * v[i].y; }
    const float rs = 1.0f / sqrtf(wave_sum(sq) / (float)C + 1e-6f);
#pragma unroll
    for (int i = 0; i < kFfgNi; ++i) if (i < ni) { v[i].x *= rs; v[i].y *= rs; }
}

// LO: also the low half of the split-precision pair, y - float(round16(y)) rounded once more (out16 and out16_lo both set)
template <class P, bool LO = false>
__device__ __forceinline__ void ffg_ln_store(const float2 (&v)[kFfgNi], int ni, int lane, const float* __restrict__ w, const float* __restrict__ b,
                                             float* out32 /* row */, typename P::elem* out16 /* row */, typename P::elem* out16_lo = nullptr) {
#pragma unroll
    for (int i = 0; i < kFfgNi; ++i) {
        if (i < ni) {
            const int c = i * 128 + lane * 2;
            const float2 lw = *(const float2*)(w + c), lb = *(const float2*)(b + c);
            const float y0 = v[i].x * lw.x + lb.x, y1 = v[i].y * lw.y + lb.y;
            if (out32) *(float2*)(out32 + c) = make_float2(y0, y1);
            if (out16) { out16[c] = to16<P>(y0); out16[c + 1] = to16<P>(y1); }
            if (LO) { out16_lo[c] = to16<P>(y0 - (float)to16<P>(y0)); out16_lo[c + 1] = to16<P>(y1 - (float)to16<P>(y1)); }
        }
    }
}

// LO: out16 is the pair tensor [row][hi C | lo C] (split-precision operands: one GEMM source whose K re-reads it, engine_ffgan.cpp)
template <class P, bool LO = false>
__global__ __launch_bounds__(256) void ffg_ln_kernel(const float* x, const float* __restrict__ w, const float* __restrict__ b, long long rows, int C,
                                                     float* out32, typename P::elem* out16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int ni = C >> 7;
    float2 v[kFfgNi];
#pragma unroll
    for (int i = 0; i < kFfgNi; ++i) v[i] = i < ni ? *(const float2*)(x + (size_t)row * C + i * 128 + lane * 2) : make_float2(0.f, 0.f);
    ffg_ln_rows(v, ni, C);
    if (LO) ffg_ln_store<P, true>(v, ni, lane, w, b, out32 ? out32 + (size_t)row * C : nullptr, out16 + (size_t)row * 2 * C, out16 + (size_t)row * 2 * C + C);
    else    ffg_ln_store<P>(v, ni, lane, w, b, out32 ? out32 + (size_t)row * C : nullptr, out16 ? out16 + (size_t)row * C : nullptr);
}

hipError_t launch_ffg_ln(int dtype, const float* x, const float* w, const float* b, int64_t rows, int C, float* out32, void* out16, hipStream_t s) {
    if (C < 128 || C > kFfgMaxDim || (C & 127)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
    if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_ln_kernel<OpBF16>), grid, blk, 0, s, x, w, b, (long long)rows, C, out32, (OpBF16::elem*)out16);
    else                  hipLaunchKernelGGL((ffg_ln_kernel<OpF16>), grid, blk, 0, s, x, w, b, (long long)rows, C, out32, (OpF16::elem*)out16);
    return hipGetLastError();
}

hipError_t launch_ffg_ln_split(int dtype, const float* x, const float* w, const float* b, int64_t rows, int C, float* out32, void* pair16, hipStream_t s) {
    if (C < 128 || C > kFfgMaxDim || (C & 127) || !pair16) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
    if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_ln_kernel<OpBF16, true>), grid, blk, 0, s, x, w, b, (long long)rows, C, out32, (OpBF16::elem*)pair16);
    else                  hipLaunchKernelGGL((ffg_ln_kernel<OpF16, true>), grid, blk, 0, s, x, w, b, (long long)rows, C, out32, (OpF16::elem*)pair16);
    return hipGetLastError();
}

// ---------------------------------------------------------------- ConvNeXt block prologue: depthwise k = 7 conv + LayerNorm (backbone.py:127-129)
// RG (ragged batch): packed row r is frame frames[r].t0 of an utterance of frames[r].T frames whose frame 0 is packed row frames[r].row0
// (one table entry per row, read through scalar registers); T is then unused.  The arithmetic per row is the same.
template <class P, bool RG, bool LO = false>
__global__ __launch_bounds__(256) void ffg_dwconv_ln_kernel(const float* __restrict__ x, const float* __restrict__ dw, const float* __restrict__ dbias,
                                                            const float* __restrict__ w, const float* __restrict__ b, int T, long long rows, int C,
                                                            const VocSeg* __restrict__ frames, typename P::elem* __restrict__ h16) {
    const int lane = threadIdx.x & 63, wave = RG ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    long long item = 0;
    int t = 0;
    if (RG) {
        const VocSeg sg = frames[row];
        item = sg.row0; t = sg.t0; T = sg.T;      // item: the utterance's first packed row
    } else {
        item = row / T;
        t = (int)(row - item * T);
    }
    const float* xi = x + (RG ? (size_t)item * C : (size_t)item * T * C);
    const int ni = C >> 7;
    float2 v[kFfgNi];
#pragma unroll
    for (int i = 0; i < kFfgNi; ++i) {
        v[i] = make_float2(0.f, 0.f);
        if (i < ni) {
            const int c = i * 128 + lane * 2;
            float2 acc = *(const float2*)(dbias + c);
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const int tt = t + j - 3;
                if (tt >= 0 && tt < T) {      // zero padding of nn.Conv1d(padding=3); wave-uniform
                    const float2 xv = *(const float2*)(xi + (size_t)tt * C + c);
                    acc.x += dw[(size_t)c * 7 + j] * xv.x;
                    acc.y += dw[(size_t)(c + 1) * 7 + j] * xv.y;
                }
            }
            v[i] = acc;
        }
    }
    ffg_ln_rows(v, ni, C);
    if (LO) ffg_ln_store<P, true>(v, ni, lane, w, b, nullptr, h16 + (size_t)row * 2 * C, h16 + (size_t)row * 2 * C + C);      // the pair row
    else    ffg_ln_store<P>(v, ni, lane, w, b, nullptr, h16 + (size_t)row * C);
}

hipError_t launch_ffg_dwconv_ln(int dtype, const float* x, const float* dw, const float* dbias, const float* w, const float* b,
                                int B, int T, int C, void* h16, hipStream_t s) {
    if (C < 128 || C > kFfgMaxDim || (C & 127)) return hipErrorInvalidValue;
    const long long rows = (long long)B * T;
    const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
    const VocSeg* none = nullptr;
    if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_dwconv_ln_kernel<OpBF16, false>), grid, blk, 0, s, x, dw, dbias, w, b, T, rows, C, none, (OpBF16::elem*)h16);
    else                  hipLaunchKernelGGL((ffg_dwconv_ln_kernel<OpF16, false>), grid, blk, 0, s, x, dw, dbias, w, b, T, rows, C, none, (OpF16::elem*)h16);
    return hipGetLastError();
}

hipError_t launch_ffg_dwconv_ln_ragged(int dtype, const float* x, const float* dw, const float* dbias, const float* w, const float* b,
                                       const VocSeg* frames, int64_t rows, int C, void* h16, hipStream_t s) {
    if (C < 128 || C > kFfgMaxDim || (C & 127) || !frames || rows < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
    if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_dwconv_ln_kernel<OpBF16, true>), grid, blk, 0, s, x, dw, dbias, w, b, 0, (long long)rows, C, frames, (OpBF16::elem*)h16);
    else                  hipLaunchKernelGGL((ffg_dwconv_ln_kernel<OpF16, true>), grid, blk, 0, s, x, dw, dbias, w, b, 0, (long long)rows, C, frames, (OpF16::elem*)h16);
    return hipGetLastError();
}

hipError_t launch_ffg_dwconv_ln_split(int dtype, const float* x, const float* dw, const float* dbias, const float* w, const float* b,
                                      int B, int T, const VocSeg* frames, int64_t rows, int C, void* pair16, hipStream_t s) {
    if (C < 128 || C > kFfgMaxDim || (C & 127) || rows < 1 || !pair16 || (!frames && rows != (int64_t)B * T)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
    const long long r = rows;
    if (frames) {
        if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_dwconv_ln_kernel<OpBF16, true, true>), grid, blk, 0, s, x, dw, dbias, w, b, 0, r, C, frames, (OpBF16::elem*)pair16);
        else                  hipLaunchKernelGGL((ffg_dwconv_ln_kernel<OpF16, true, true>), grid, blk, 0, s, x, dw, dbias, w, b, 0, r, C, frames, (OpF16::elem*)pair16);
    } else {
        if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_dwconv_ln_kernel<OpBF16, false, true>), grid, blk, 0, s, x, dw, dbias, w, b, T, r, C, frames, (OpBF16::elem*)pair16);
        else                  hipLaunchKernelGGL((ffg_dwconv_ln_kernel<OpF16, false, true>), grid, blk, 0, s, x, dw, dbias, w, b, T, r, C, frames, (OpF16::elem*)pair16);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------- split mode: the stem's im2col rows and the GELU between the pointwise convs
// One block = 64 frames of one utterance, as the Vocos im2col (vocos_kernels.hip): the (M x 70) mel tile is read with frames contiguous
// and written as the pair rows [frame][hi: [tap][channel] | lo: [tap][channel]].  RG: block = one entry of the 64-frame tile table.
template <class P, bool RG>
__global__ __launch_bounds__(256) void ffg_im2col7_split_kernel(const float* __restrict__ mel, const VocSeg* __restrict__ tiles, int M, int Tpad,
                                                                typename P::elem* __restrict__ a16) {
    extern __shared__ float tile[];           // [M][72]
    int T = Tpad, t0 = blockIdx.x * 64, item = blockIdx.y;
    size_t row0 = (size_t)item * Tpad;
    if (RG) {
        const VocSeg sg = tiles[blockIdx.x];
        T = sg.T; t0 = sg.t0; item = sg.item; row0 = (size_t)sg.row0;
    }
    const float* src = mel + (size_t)item * M * Tpad;
    for (int i = threadIdx.x; i < M * 70; i += 256) {
        const int c = i / 70, k = i - c * 70;
        const int t = t0 + k - 3;
        tile[c * 72 + k] = (t >= 0 && t < T) ? src[(size_t)c * Tpad + t] : 0.0f;
    }
    __syncthreads();
    const int K = 7 * M;
    for (int i = threadIdx.x; i < 64 * K; i += 256) {
        const int f = i / K, r = i - f * K;
        const int j = r / M, c = r - j * M;
        if (t0 + f < T) {
            const float v = tile[c * 72 + f + j];
            const typename P::elem hi = to16<P>(v);
            const size_t o = (row0 + t0 + f) * 2 * K + r;
            a16[o] = hi;
            a16[o + K] = to16<P>(v - (float)hi);
        }
    }
}

hipError_t launch_ffg_im2col7_split(int dtype, const float* mel, int B, int M, int T, const VocSeg* tiles, int n_tiles, void* a16, hipStream_t s) {
    const size_t lds = (size_t)M * 72 * 4;
    if (lds > 64 * 1024 || M < 1 || T < 1 || B < 1 || B > 65535 || (tiles && n_tiles < 1) || !a16) return hipErrorInvalidValue;
    const dim3 blk(256);
    if (tiles) {
        const dim3 grid((unsigned)n_tiles);
        if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_im2col7_split_kernel<OpBF16, true>), grid, blk, lds, s, mel, tiles, M, T, (OpBF16::elem*)a16);
        else                  hipLaunchKernelGGL((ffg_im2col7_split_kernel<OpF16, true>), grid, blk, lds, s, mel, tiles, M, T, (OpF16::elem*)a16);
    } else {
        const dim3 grid((unsigned)((T + 63) / 64), (unsigned)B);
        if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_im2col7_split_kernel<OpBF16, false>), grid, blk, lds, s, mel, tiles, M, T, (OpBF16::elem*)a16);
        else                  hipLaunchKernelGGL((ffg_im2col7_split_kernel<OpF16, false>), grid, blk, lds, s, mel, tiles, M, T, (OpF16::elem*)a16);
    }
    return hipGetLastError();
}

// nn.GELU() with libm's erff (the A&S polynomial of common.h is good to 4.7e-7 absolute: fine under a 16-bit rounding, not beside a
// pair that carries 22 bits); four elements per thread; x: [rows][F], the pair rows [rows][hi F | lo F], F a multiple of 4
template <class P>
__global__ __launch_bounds__(256) void ffg_gelu_split_kernel(const float* __restrict__ x, long long n4, int F4, uint2* __restrict__ u16) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long long row = i / F4, o = row * 2 * F4 + (i - row * F4);
    const float4 v = *(const float4*)(x + i * 4);
    float g[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = 0.5f * g[k] * (1.0f + erff(g[k] * 0.70710678118654752f));
    asm volatile("" : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]));      // the pair splits the fp32 VALUE: no fma of the last product into g - hi
    u16[o] = pack4<P>(g[0], g[1], g[2], g[3]);
    u16[o + F4] = pack4<P>(g[0] - (float)to16<P>(g[0]), g[1] - (float)to16<P>(g[1]), g[2] - (float)to16<P>(g[2]), g[3] - (float)to16<P>(g[3]));
}

hipError_t launch_ffg_gelu_split(int dtype, const float* x, int64_t rows, int F, void* u16, hipStream_t s) {
    if (rows < 1 || F < 4 || (F & 3) || !u16) return hipErrorInvalidValue;
    const long long n4 = rows * (F / 4);
    const dim3 grid((unsigned)((n4 + 255) / 256)), blk(256);
    if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_gelu_split_kernel<OpBF16>), grid, blk, 0, s, x, n4, F / 4, (uint2*)u16);
    else                  hipLaunchKernelGGL((ffg_gelu_split_kernel<OpF16>), grid, blk, 0, s, x, n4, F / 4, (uint2*)u16);
    return hipGetLastError();
}

template <class P>
__global__ __launch_bounds__(256) void ffg_pack_rows_split_kernel(const float* __restrict__ src, int cout, int cin, int taps, int parts,
                                                                  typename P::elem* __restrict__ dst) {
    const size_t K = (size_t)taps * cin, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)cout * K) return;
    const int co = (int)(idx / K), r = (int)(idx - (size_t)co * K), j = r / cin, c = r - j * cin;
    const float w = src[((size_t)co * cin + c) * taps + j];
    const typename P::elem hi = to16<P>(w);
    const typename P::elem lo = to16<P>(w - (float)hi);
    typename P::elem* row = dst + (size_t)co * parts * K;
    row[r] = hi; row[K + r] = hi; row[2 * K + r] = lo;
    if (parts == 4) row[3 * K + r] = lo;
}

hipError_t launch_ffg_pack_rows_split(int dtype, const float* src, int cout, int cin, int taps, int parts, void* dst, hipStream_t s) {
    if (cout < 1 || cin < 1 || taps < 1 || (parts != 3 && parts != 4)) return hipErrorInvalidValue;
    const size_t n = (size_t)cout * cin * taps;
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_pack_rows_split_kernel<OpBF16>), grid, blk, 0, s, src, cout, cin, taps, parts, (OpBF16::elem*)dst);
    else                  hipLaunchKernelGGL((ffg_pack_rows_split_kernel<OpF16>), grid, blk, 0, s, src, cout, cin, taps, parts, (OpF16::elem*)dst);
    return hipGetLastError();
}

// ---------------------------------------------------------------- head: implicit-GEMM convolution (ffgan_launch.h)
// 4 waves; wave w owns frames 32 w .. 32 w + 31 of the tile (two 16-frame B operands) and all CW * 16 output channels of the block.
// Fragment maps of the 16x16x32 MFMA (common.h): A = weights, lane l holds W[co = l & 15][k = 8 (l >> 4) .. + 8]; B = patch rows, lane l
// holds a[frame = l & 15][the same k]; D: lane l, register r = out[co = 4 (l >> 4) + r][frame = l & 15] -- four consecutive output
// channels of one frame, one 16-byte store.
// RG (ragged batch, a.utt): the block's item owns the packed rows row0 .. row0 + L of its own length L; a block past that end exits
// before anything else (block-uniform).  Everything after that is the dense kernel on that item alone.
// Parts of a split-precision operand in the head (ffgan_launch.h): f16 two (hi, lo; lo * lo = 2^-22 of a product is dropped), bf16 three
template <class P> constexpr int ffg_split_parts() { return std::is_same<P, OpBF16>::value ? 3 : 2; }

// SPLIT (launch_ffg_conv_split): the patch is two planes (bf16: three), hi at 0 and the next part every rows * S bytes, of
// kc = min(cin, kFfgSplitKc) channels; the fp32 input is split while staging (after the SiLU, or as it is with a.in_raw); the fragment
// stream carries every k-step's parts in the same order; three (bf16: six) MFMAs per fragment pair in a fixed order.  Everything else -- tiles, halo, ragged exit, epilogue -- is the code above.
template <class P, bool IN16, int EPI, int CW, bool RG, bool SPLIT = false>
__global__ __launch_bounds__(256) void ffg_conv_kernel(FfgConvArgs a) {
    static_assert(!SPLIT || (!IN16 && EPI != FFG_SILU16), "split mode stages fp32 inputs and stores fp32");
    extern __shared__ __align__(16) unsigned char patch[];      // [rows][kc * 2 + 16 bytes] (SPLIT: two such planes)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, fl = lane & 15;
    const int t0 = blockIdx.x * kFfgFrames, item = blockIdx.z, ct0 = blockIdx.y * CW;
    const int cin = a.cin, cout = a.cout, taps = a.taps, dil = a.dil;
    int L = a.L;
    size_t row0 = (size_t)item * L;      // the item's first row
    if (RG) {
        const VocUtt u = a.utt[item];
        L = u.T * a.up;
        row0 = (size_t)u.row0 * a.up;
        if (t0 >= L) return;
    }
    const int kc = cin < (SPLIT ? kFfgSplitKc : 128) ? cin : (SPLIT ? kFfgSplitKc : 128), lg = 31 - __builtin_clz(kc);
    const int S = kc * 2 + 16, halo = (taps >> 1) * dil, rows = kFfgFrames + 2 * halo;
    const int nchunks = cin / kc, ksc = (taps * kc + 31) >> 5;
    const size_t in_base = row0 * cin;

    f32x4_t acc[2][CW];
#pragma unroll
    for (int fw = 0; fw < 2; ++fw)
#pragma unroll
        for (int cw = 0; cw < CW; ++cw) acc[fw][cw] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    constexpr int PL = SPLIT ? ffg_split_parts<P>() : 1;    // planes of the patch = fragments per k-step
    constexpr int WL = 64 * PL;                             // uint4 per k-step of one tile
    const uint4* wf = (const uint4*)a.wfrag + ((size_t)ct0 * nchunks * ksc) * WL + lane;
    const size_t wf_tile = (size_t)nchunks * ksc * WL;      // uint4 per 16-channel tile
    const int plane = SPLIT ? rows * S : 0;                 // bytes between two planes

    for (int ch = 0; ch < nchunks; ++ch) {
        if (ch) __syncthreads();
        if (SPLIT) {
            const int per = kc >> 2, n = rows * per;
            const float* src = a.in32 + in_base + (size_t)ch * kc;
            const bool raw = a.in_raw != 0;      // block-uniform
            for (int i = threadIdx.x; i < n; i += 256) {
                const int r = i / per, c4 = i - r * per, t = t0 - halo + r;
                uint2 hi = make_uint2(0u, 0u), lo = make_uint2(0u, 0u), l3 = make_uint2(0u, 0u);
                if (t >= 0 && t < L) {
                    const float4 x = *(const float4*)(src + (size_t)t * cin + c4 * 4);
                    float v0 = raw ? x.x : silu_fast(x.x), v1 = raw ? x.y : silu_fast(x.y), v2 = raw ? x.z : silu_fast(x.z), v3 = raw ? x.w : silu_fast(x.w);
                    asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));      // split the fp32 VALUE (no fma of silu's product into v - hi)
                    hi = pack4<P>(v0, v1, v2, v3);
                    v0 -= (float)to16<P>(v0); v1 -= (float)to16<P>(v1); v2 -= (float)to16<P>(v2); v3 -= (float)to16<P>(v3);      // exact in fp32
                    lo = pack4<P>(v0, v1, v2, v3);
                    if (PL == 3) l3 = pack4<P>(v0 - (float)to16<P>(v0), v1 - (float)to16<P>(v1), v2 - (float)to16<P>(v2), v3 - (float)to16<P>(v3));
                }
                *(uint2*)(patch + r * S + c4 * 8) = hi;
                *(uint2*)(patch + plane + r * S + c4 * 8) = lo;
                if (PL == 3) *(uint2*)(patch + 2 * plane + r * S + c4 * 8) = l3;
            }
        } else if (IN16) {
            const int per = kc >> 3, n = rows * per;
            const typename P::elem* src = (const typename P::elem*)a.in16 + in_base + (size_t)ch * kc;
            for (int i = threadIdx.x; i < n; i += 256) {
                const int r = i / per, c8 = i - r * per, t = t0 - halo + r;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (t >= 0 && t < L) v = *(const uint4*)(src + (size_t)t * cin + c8 * 8);
                *(uint4*)(patch + r * S + c8 * 16) = v;
            }
        } else {
            const int per = kc >> 2, n = rows * per;
            const float* src = a.in32 + in_base + (size_t)ch * kc;
            for (int i = threadIdx.x; i < n; i += 256) {
                const int r = i / per, c4 = i - r * per, t = t0 - halo + r;
                uint2 v = make_uint2(0u, 0u);
                if (t >= 0 && t < L) {
                    const float4 x = *(const float4*)(src + (size_t)t * cin + c4 * 4);
                    v = pack4<P>(silu_fast(x.x), silu_fast(x.y), silu_fast(x.z), silu_fast(x.w));
                }
                *(uint2*)(patch + r * S + c4 * 8) = v;
            }
        }
        __syncthreads();
        const uint4* wc = wf + (size_t)ch * ksc * WL;
        for (int ks = 0; ks < ksc; ++ks) {
            const int kk = ks * 32 + 8 * g;
            int tap = kk >> lg;
            const int ci = kk & (kc - 1);
            tap = tap < taps ? tap : taps - 1;      // zero-weight padding of K: any finite row
            uint4 wv[CW], wl[SPLIT ? CW : 1], w3[PL == 3 ? CW : 1];
#pragma unroll
            for (int cw = 0; cw < CW; ++cw) wv[cw] = wc[(size_t)cw * wf_tile + (size_t)ks * WL];
            if (SPLIT) {
#pragma unroll
                for (int cw = 0; cw < CW; ++cw) wl[cw] = wc[(size_t)cw * wf_tile + (size_t)ks * WL + 64];
            }
            if (PL == 3) {
#pragma unroll
                for (int cw = 0; cw < CW; ++cw) w3[cw] = wc[(size_t)cw * wf_tile + (size_t)ks * WL + 128];
            }
            const unsigned char* prow = patch + (wave * 32 + fl + tap * dil) * S + ci * 2;
#pragma unroll
            for (int fw = 0; fw < 2; ++fw) {
                const uint4 bv = *(const uint4*)(prow + fw * 16 * S);
                if (SPLIT) {
                    const uint4 bl = *(const uint4*)(prow + plane + fw * 16 * S);
                    uint4 b3 = make_uint4(0u, 0u, 0u, 0u);
                    if (PL == 3) b3 = *(const uint4*)(prow + 2 * plane + fw * 16 * S);
#pragma unroll
                    for (int cw = 0; cw < CW; ++cw) {
                        acc[fw][cw] = P::mfma16(as_vec8<P>(wv[cw]), as_vec8<P>(bv), acc[fw][cw]);
                        acc[fw][cw] = P::mfma16(as_vec8<P>(wv[cw]), as_vec8<P>(bl), acc[fw][cw]);
                        acc[fw][cw] = P::mfma16(as_vec8<P>(wl[cw]), as_vec8<P>(bv), acc[fw][cw]);
                        if (PL == 3) {      // (hi, mid, lo): the mid * mid product and the two with a lo part
                            acc[fw][cw] = P::mfma16(as_vec8<P>(wl[cw]), as_vec8<P>(bl), acc[fw][cw]);
                            acc[fw][cw] = P::mfma16(as_vec8<P>(wv[cw]), as_vec8<P>(b3), acc[fw][cw]);
                            acc[fw][cw] = P::mfma16(as_vec8<P>(w3[cw]), as_vec8<P>(bv), acc[fw][cw]);
                        }
                    }
                } else {
#pragma unroll
                    for (int cw = 0; cw < CW; ++cw) acc[fw][cw] = P::mfma16(as_vec8<P>(wv[cw]), as_vec8<P>(bv), acc[fw][cw]);
                }
            }
        }
    }

#pragma unroll
    for (int fw = 0; fw < 2; ++fw) {
        const int t = t0 + wave * 32 + fw * 16 + fl;
        if (t >= L) continue;
#pragma unroll
        for (int cw = 0; cw < CW; ++cw) {
            const int co = (ct0 + cw) * 16 + 4 * g;
            const size_t o = (row0 + t) * cout + co;
            const float4 bb = *(const float4*)(a.bias + co);
            float4 y = make_float4(acc[fw][cw][0] + bb.x, acc[fw][cw][1] + bb.y, acc[fw][cw][2] + bb.z, acc[fw][cw][3] + bb.w);
            if (EPI == FFG_F32) {
                *(float4*)(a.out32 + o) = y;
            } else if (EPI == FFG_SILU16) {
                *(uint2*)((typename P::elem*)a.out16 + o) = pack4<P>(silu_fast(y.x), silu_fast(y.y), silu_fast(y.z), silu_fast(y.w));
            } else {
                const float4 r = *(const float4*)(a.res32 + o);
                y.x += r.x; y.y += r.y; y.z += r.z; y.w += r.w;
                if (a.out32) *(float4*)(a.out32 + o) = y;
                if (a.mean) {
                    float4 m = y;
                    if (!a.mean_first) { const float4 p = *(const float4*)(a.mean + o); m.x += p.x; m.y += p.y; m.z += p.z; m.w += p.w; }
                    const float sc = a.mean_scale;
                    *(float4*)(a.mean + o) = make_float4(m.x * sc, m.y * sc, m.z * sc, m.w * sc);
                }
            }
        }
    }
}

bool ffg_conv_supported(int cin, int cout, int taps, int dil) {
    const bool cin_ok = cin == 16 || cin == 32 || cin == 64 || (cin >= 128 && cin % 128 == 0);
    return cin_ok && cout >= 16 && cout % 16 == 0 && taps >= 1 && (taps & 1) && taps <= kFfgMaxTaps && dil >= 1 && (taps / 2) * dil <= kFfgMaxHalo;
}

template <class P, bool IN16, int EPI, bool RG, bool SPLIT = false>
static hipError_t ffg_conv_rg(const FfgConvArgs& a, hipStream_t s) {
    const int tiles = a.cout / 16, cw = tiles % 4 == 0 ? 4 : tiles % 2 == 0 ? 2 : 1;
    constexpr int PL = SPLIT ? ffg_split_parts<P>() : 1;
    const int kc = ffg_kc(a.cin, PL), rows = kFfgFrames + 2 * (a.taps / 2) * a.dil;
    const size_t lds = (size_t)rows * (kc * 2 + 16) * PL;
    if (PL == 3) {      // three planes at the largest halo exceed the 64 KB a kernel gets by default: opt in per device and instantiation
        constexpr int kMaxLds = 3 * (kFfgFrames + 2 * kFfgMaxHalo) * (kFfgSplitKc * 2 + 16);
        // remembered per device id; setting the attribute again is harmless, so two threads that both find the flag clear both set it,
        // and a device id beyond the table sets it at every launch
        static std::atomic<bool> attr_done_dev[64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0) return hipErrorInvalidDevice;
        const bool known = dev < 64;
        if (!known || !attr_done_dev[dev].load(std::memory_order_acquire)) {
            for (const void* fn : {(const void*)ffg_conv_kernel<P, IN16, EPI, 4, RG, SPLIT>, (const void*)ffg_conv_kernel<P, IN16, EPI, 2, RG, SPLIT>,
                                   (const void*)ffg_conv_kernel<P, IN16, EPI, 1, RG, SPLIT>}) {
                const hipError_t he = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
                if (he != hipSuccess) return he;
            }
            if (known) attr_done_dev[dev].store(true, std::memory_order_release);
        }
        if (lds > (size_t)kMaxLds) return hipErrorInvalidValue;
    } else if (lds > 64 * 1024) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.L + kFfgFrames - 1) / kFfgFrames), (unsigned)(tiles / cw), (unsigned)a.n_items), blk(256);
    if (cw == 4)      hipLaunchKernelGGL((ffg_conv_kernel<P, IN16, EPI, 4, RG, SPLIT>), grid, blk, lds, s, a);
    else if (cw == 2) hipLaunchKernelGGL((ffg_conv_kernel<P, IN16, EPI, 2, RG, SPLIT>), grid, blk, lds, s, a);
    else              hipLaunchKernelGGL((ffg_conv_kernel<P, IN16, EPI, 1, RG, SPLIT>), grid, blk, lds, s, a);
    return hipGetLastError();
}

template <class P, bool IN16, int EPI, bool SPLIT = false>
static hipError_t ffg_conv_cw(const FfgConvArgs& a, hipStream_t s) {
    return a.utt ? ffg_conv_rg<P, IN16, EPI, true, SPLIT>(a, s) : ffg_conv_rg<P, IN16, EPI, false, SPLIT>(a, s);
}

template <class P>
static hipError_t ffg_conv_dt(const FfgConvArgs& a, hipStream_t s) {
    const bool in16 = a.in16 != nullptr;
    if (a.epi == FFG_F32 && a.out32) return in16 ? ffg_conv_cw<P, true, FFG_F32>(a, s) : ffg_conv_cw<P, false, FFG_F32>(a, s);
    if (a.epi == FFG_SILU16 && a.out16 && !in16) return ffg_conv_cw<P, false, FFG_SILU16>(a, s);
    if (a.epi == FFG_RES && a.res32 && (a.out32 || a.mean) && in16) return ffg_conv_cw<P, true, FFG_RES>(a, s);
    return hipErrorInvalidValue;
}

hipError_t launch_ffg_conv(int dtype, const FfgConvArgs& a, hipStream_t s) {
    if (!ffg_conv_supported(a.cin, a.cout, a.taps, a.dil) || (a.in32 != nullptr) == (a.in16 != nullptr) || !a.wfrag || !a.bias) return hipErrorInvalidValue;
    if (a.L < 1 || a.n_items < 1 || a.n_items > 65535 || (a.utt && a.up < 1) || a.in_raw) return hipErrorInvalidValue;
    return dtype == DT_BF16 ? ffg_conv_dt<OpBF16>(a, s) : ffg_conv_dt<OpF16>(a, s);
}

template <class P>
static hipError_t ffg_conv_split_dt(const FfgConvArgs& a, hipStream_t s) {
    if (a.epi == FFG_F32 && a.out32) return ffg_conv_cw<P, false, FFG_F32, true>(a, s);
    if (a.epi == FFG_RES && a.res32 && (a.out32 || a.mean) && !a.in_raw) return ffg_conv_cw<P, false, FFG_RES, true>(a, s);
    return hipErrorInvalidValue;
}

hipError_t launch_ffg_conv_split(int dtype, const FfgConvArgs& a, hipStream_t s) {
    if (!ffg_conv_supported(a.cin, a.cout, a.taps, a.dil) || !a.in32 || a.in16 || !a.wfrag || !a.bias) return hipErrorInvalidValue;
    if (a.L < 1 || a.n_items < 1 || a.n_items > 65535 || (a.utt && a.up < 1)) return hipErrorInvalidValue;
    return dtype == DT_BF16 ? ffg_conv_split_dt<OpBF16>(a, s) : ffg_conv_split_dt<OpF16>(a, s);
}

// ---------------------------------------------------------------- st_finalize: weight norm and packing
__global__ __launch_bounds__(256) void ffg_wn_scale_kernel(const float* __restrict__ v, const float* __restrict__ g, int inner, float* __restrict__ scale) {
    __shared__ double part[256];
    const float* row = v + (size_t)blockIdx.x * inner;
    double sq = 0.0;
    for (int i = threadIdx.x; i < inner; i += 256) sq += (double)row[i] * (double)row[i];
    part[threadIdx.x] = sq;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) scale[blockIdx.x] = (float)((double)g[blockIdx.x] / sqrt(part[0]));
}

hipError_t launch_ffg_wn_scale(const float* v, const float* g, int rows, int inner, float* scale, hipStream_t s) {
    hipLaunchKernelGGL(ffg_wn_scale_kernel, dim3(rows), dim3(256), 0, s, v, g, inner, scale);
    return hipGetLastError();
}

// one thread per 16-bit element of the fragment stream: [tile = co / 16][chunk][k-step][lane][8]
// SPLIT: chunks of kFfgSplitKc channels and [tile][chunk][k-step][part][lane][8]; a thread writes every part of its element (n counts the hi elements)
template <class P, bool SPLIT = false>
__global__ __launch_bounds__(256) void ffg_pack_conv_kernel(const float* __restrict__ v, const float* __restrict__ scale, int cout, int cin, int taps,
                                                            int u, long long n, typename P::elem* __restrict__ dst) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    int srow = 0;
    const long long src = ffg_frag_source(idx, cout, cin, taps, u, SPLIT, &srow);
    float val = 0.0f;
    if (src >= 0) val = v[src] * (scale ? scale[srow] : 1.0f);
    // the folded weight is an fp32 value (a product rounded to fp32, as this kernel always computed it) before it is rounded to 16 bits
    // or split into its pair: no v_fma_mixlo of the product into the conversion (common.h: scale_pack4, scale_pack4_lo)
    asm volatile("" : "+v"(val));
    if (SPLIT) {
        constexpr int PL = ffg_split_parts<P>();
        const typename P::elem hi = to16<P>(val);
        const float r1 = val - (float)hi;
        const typename P::elem mid = to16<P>(r1);
        dst[ffg_frag_offset(idx, PL, 0)] = hi;
        dst[ffg_frag_offset(idx, PL, 1)] = mid;
        if (PL == 3) dst[ffg_frag_offset(idx, PL, 2)] = to16<P>(r1 - (float)mid);
    } else {
        dst[idx] = to16<P>(val);
    }
}

hipError_t launch_ffg_pack_conv(int dtype, const float* v, const float* scale, int cout, int cin, int taps, int transposed, void* wfrag, hipStream_t s,
                                bool split) {
    if (!ffg_conv_supported(cin, cout, taps, 1) || (transposed && (taps != 3 || cout % transposed != 0))) return hipErrorInvalidValue;
    const int planes = split ? ffg_split_planes(dtype) : 1;
    const long long n = (long long)(ffg_frag_bytes(cout, cin, taps, planes) / (2 * planes));
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    if (split) {
        if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_pack_conv_kernel<OpBF16, true>), grid, blk, 0, s, v, scale, cout, cin, taps, transposed, n, (OpBF16::elem*)wfrag);
        else                  hipLaunchKernelGGL((ffg_pack_conv_kernel<OpF16, true>), grid, blk, 0, s, v, scale, cout, cin, taps, transposed, n, (OpF16::elem*)wfrag);
        return hipGetLastError();
    }
    if (dtype == DT_BF16) hipLaunchKernelGGL((ffg_pack_conv_kernel<OpBF16>), grid, blk, 0, s, v, scale, cout, cin, taps, transposed, n, (OpBF16::elem*)wfrag);
    else                  hipLaunchKernelGGL((ffg_pack_conv_kernel<OpF16>), grid, blk, 0, s, v, scale, cout, cin, taps, transposed, n, (OpF16::elem*)wfrag);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void ffg_pack_post_kernel(const float* __restrict__ v, const float* __restrict__ scale, int cin, int taps, float* __restrict__ dst) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= cin * taps) return;
    const int j = idx / cin, ci = idx - j * cin;
    dst[idx] = v[(size_t)ci * taps + j] * scale[0];
}

hipError_t launch_ffg_pack_post(const float* v, const float* scale, int cin, int taps, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(ffg_pack_post_kernel, dim3((cin * taps + 255) / 256), dim3(256), 0, s, v, scale, cin, taps, dst);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void ffg_tile_bias_kernel(const float* __restrict__ bias, int cout, int n, float* __restrict__ dst) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n) dst[idx] = bias[idx % cout];
}

hipError_t launch_ffg_tile_bias(const float* bias, int cout, int u, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(ffg_tile_bias_kernel, dim3((cout * u + 255) / 256), dim3(256), 0, s, bias, cout, cout * u, dst);
    return hipGetLastError();
}

// ---------------------------------------------------------------- SiLU -> conv_post (C -> 1) -> tanh, fp32 (head.py:245-247)
// One block = 256 samples of one item; 16 channels at a time: silu(x) of the 256 + taps - 1 rows in LDS (row pitch 20 floats: the
// 16-byte reads of 16 consecutive rows fall into 16 different bank slots), one thread per sample.
// RG (ragged batch): x and pre hold packed rows, the item's own L = utt[item].T * hop samples from row utt[item].row0 * hop; the audio is
// padded to Lpad samples per item and a block past the item's end writes its zeros and exits before anything else (block-uniform).
constexpr int kFfgPostPitch = 20;
template <bool RG>
__global__ __launch_bounds__(256) void ffg_post_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const VocUtt* __restrict__ utt, int hop, int Lpad, int C, int taps,
                                                       float* __restrict__ pre, float* __restrict__ audio) {
    __shared__ __align__(16) float tile[(256 + kFfgMaxTaps - 1) * kFfgPostPitch];
    __shared__ __align__(16) float wl[kFfgMaxTaps * 16];
    const int t0 = blockIdx.x * 256, item = blockIdx.y, halo = taps >> 1, rows = 256 + taps - 1;
    int L = Lpad;
    size_t row0 = (size_t)item * L;
    if (RG) {
        const VocUtt u = utt[item];
        L = u.T * hop;
        row0 = (size_t)u.row0 * hop;
        if (t0 >= L) {
            const int t = t0 + threadIdx.x;
            if (t < Lpad) audio[(size_t)item * Lpad + t] = 0.0f;
            return;
        }
    }
    const float* xi = x + row0 * C;
    float acc = 0.0f;
    for (int c0 = 0; c0 < C; c0 += 16) {
        if (c0) __syncthreads();
        for (int i = threadIdx.x; i < rows * 4; i += 256) {
            const int r = i >> 2, q = i & 3, t = t0 - halo + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t >= 0 && t < L) {
                const float4 xv = *(const float4*)(xi + (size_t)t * C + c0 + q * 4);
                v = make_float4(silu_f(xv.x), silu_f(xv.y), silu_f(xv.z), silu_f(xv.w));
            }
            *(float4*)(tile + r * kFfgPostPitch + q * 4) = v;
        }
        for (int i = threadIdx.x; i < taps * 16; i += 256) wl[i] = w[(size_t)(i >> 4) * C + c0 + (i & 15)];
        __syncthreads();
        for (int j = 0; j < taps; ++j) {
            const float* row = tile + (threadIdx.x + j) * kFfgPostPitch;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 xv = *(const float4*)(row + q * 4), wv = *(const float4*)(wl + j * 16 + q * 4);
                acc += xv.x * wv.x + xv.y * wv.y + xv.z * wv.z + xv.w * wv.w;
            }
        }
    }
    const int t = t0 + threadIdx.x;
    if (t < L) {
        const float y = acc + bias[0];
        if (pre) pre[row0 + t] = y;
        audio[(size_t)item * Lpad + t] = tanhf(y);
    } else if (RG && t < Lpad) {
        audio[(size_t)item * Lpad + t] = 0.0f;
    }
}

hipError_t launch_ffg_post(const float* x, const float* w, const float* bias, int n_items, int L, int C, int taps, float* pre, float* audio, hipStream_t s) {
    if (C < 16 || (C & 15) || taps < 1 || !(taps & 1) || taps > kFfgMaxTaps || n_items < 1 || n_items > 65535 || L < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ffg_post_kernel<false>, dim3((unsigned)((L + 255) / 256), (unsigned)n_items), dim3(256), 0, s, x, w, bias, (const VocUtt*)nullptr, 1, L, C,
                       taps, pre, audio);
    return hipGetLastError();
}

hipError_t launch_ffg_post_ragged(const float* x, const float* w, const float* bias, const VocUtt* utt, int hop, int n_items, int L, int C, int taps,
                                  float* pre, float* audio, hipStream_t s) {
    if (C < 16 || (C & 15) || taps < 1 || !(taps & 1) || taps > kFfgMaxTaps || n_items < 1 || n_items > 65535 || L < 1 || !utt || hop < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ffg_post_kernel<true>, dim3((unsigned)((L + 255) / 256), (unsigned)n_items), dim3(256), 0, s, x, w, bias, utt, hop, L, C, taps, pre, audio);
    return hipGetLastError();
}

}  // namespace st
