// The fp32 MFMA tile (v_mfma_f32_32x32x2_f32: bit-for-bit a k-ordered fp32 FMA chain) behind the style-encoder, duration-
// predictor, Vocos-training and discriminator kernels, written once: the lane / wave mapping (64 x 64, and 32 x 128 for GEMMs of
// 32 rows), the K loop, the walk over the D fragment, the split-K weight-gradient kernel with its split rule, plane sum and
// launcher, and two small helpers (grid_1d, block_sum256).  The conv kernels (sd_conv_kernel, pd_conv_kernel, rd_conv_kernel) keep
// their own operand staging and epilogues (sd_conv_kernel may run four such chains side by side over K: SdConvArgs::chains).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace st {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int kTile = 64, kTileChunk = 16;      // output tile 64 rows x 64 columns; the convs stage 16 input channels per K step

// One block = 4 waves = a 64 x 64 output tile; wave w owns the 32 x 32 sub-tile at (rows 32 wco, columns 32 wt).  MFMA 32x32x2
// f32 operands: lane l holds A[i = r][k = h] and B[k = h][j = r], r = l & 31, h = l >> 5; D: row (i & 3) + 8 (i >> 2) + 4 h of
// accumulator element i, column r.
struct TileLane { int r, h, wco, wt; };

__device__ __forceinline__ TileLane tile_lane() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return {lane & 31, lane >> 5, wave & 1, wave >> 1};
}

__device__ __forceinline__ f32x16 tile_zero() {
    f32x16 acc;
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    return acc;
}

// acc += A[rows of this wave][0 .. KC) B[0 .. KC)[columns of this wave], k ascending in pairs.  As: the A tile in LDS, row-major
// with row stride a_stride; b(k, column): the B operand from LDS.
template <int KC, int UNROLL, typename BFetch>
__device__ __forceinline__ void tile_mfma(f32x16& acc, const float* As, int a_stride, const TileLane& l, BFetch b) {
    const float* a_row = As + (l.wco * 32 + l.r) * a_stride;
    const int col = l.wt * 32 + l.r;
#pragma unroll UNROLL
    for (int kk = 0; kk < KC; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_row[kk + l.h], b(kk + l.h, col), acc, 0, 0, 0);
}

// f(row of the 64 x 64 tile, value) for the 16 accumulator elements of this lane (their column is 32 wt + r)
template <typename F>
__device__ __forceinline__ void tile_for_each(const f32x16& acc, const TileLane& l, F f) {
    for (int i = 0; i < 16; ++i) f(l.wco * 32 + (i & 3) + 8 * (i >> 2) + 4 * l.h, acc[i]);
}

// The same MFMA on a 32 x 128 tile, for GEMMs whose M is 32 (the band convs of the resolution discriminator): four waves side by
// side, wave w owns rows 0..31 x columns 32 w .. 32 w + 31.  Operand and D layout as above with wco = 0, wt = the wave.
constexpr int kWideRows = 32, kWideCols = 128;

__device__ __forceinline__ TileLane wide_lane() {
    const int lane = threadIdx.x & 63;
    return {lane & 31, lane >> 5, 0, (int)(threadIdx.x >> 6)};
}

inline unsigned grid_1d(int64_t n, int64_t cap) {      // blocks of 256 threads for a grid-stride loop over n elements
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b < cap ? (b > 0 ? b : 1) : cap);
}

// Sum of v over the 256 threads of the block in a fixed LDS tree (red: 256 floats); every thread gets the sum.
__device__ __forceinline__ float block_sum256(float* red, float v) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    return red[0];
}

// ---- weight gradient: dW[co][n] = sum_f dY[f][co] X'[f][n], a TN GEMM over the frames f ----------------------------------
// One block = a 64 (co) x 64 (n) tile of one split s (blockIdx.z): frames [s * fs, min((s + 1) * fs, frames)), 32 per LDS chunk;
// A[i = co][k = frame], B[k = frame][j = n].  A thread stages one frame column of both operands (256 % 32 == 0), so the frame
// decomposition happens once per thread and chunk.  Src supplies the operands:
//   int cout(), n(); int64_t frames();  Frame frame(f);  float dy(Frame, co);  float x(Frame, n)  (the gathered input, 0 outside it)
constexpr int kWgChunk = 32, kWgMaxSplits = 32;

template <typename Src>
__global__ __launch_bounds__(256) void wgrad_kernel(Src src, int fs, float* __restrict__ dst) {
    constexpr int LS = kWgChunk + 1;
    __shared__ float Ys[kTile * LS];
    __shared__ float Xs[kTile * LS];
    const int tid = threadIdx.x, kf = tid & 31;
    const TileLane l = tile_lane();
    const int n0 = blockIdx.x * kTile, co0 = blockIdx.y * kTile, s = blockIdx.z;
    const int Cout = src.cout(), N = src.n();
    const int64_t F = src.frames(), f_lo = (int64_t)s * fs, f_hi = f_lo + fs < F ? f_lo + fs : F;
    f32x16 acc = tile_zero();
    for (int64_t f0 = f_lo; f0 < f_hi; f0 += kWgChunk) {
        const bool ok = f0 + kf < f_hi;
        const auto fr = src.frame(ok ? f0 + kf : 0);
        for (int row = tid >> 5; row < kTile; row += 8) {
            float yv = 0.0f, xv = 0.0f;
            if (ok) {
                if (co0 + row < Cout) yv = src.dy(fr, co0 + row);
                if (n0 + row < N) xv = src.x(fr, n0 + row);
            }
            Ys[row * LS + kf] = yv;
            Xs[row * LS + kf] = xv;
        }
        __syncthreads();
        tile_mfma<kWgChunk, kWgChunk / 2>(acc, Ys, LS, l, [&](int k, int col) { return Xs[col * LS + k]; });
        __syncthreads();
    }
    const int n = n0 + l.wt * 32 + l.r;
    if (n >= N) return;
    float* out = dst + (size_t)s * Cout * N;
    tile_for_each(acc, l, [&](int row, float v) {
        if (co0 + row < Cout) out[(size_t)(co0 + row) * N + n] = v;
    });
}

// The split, fixed by the shape alone (deterministic): enough splits to give ~256 blocks, each split >= 128 frames and a
// multiple of the chunk.  Returns the planes, *fs = frames per plane.
inline int wgrad_split(int64_t frames, int Cout, int N, int* fs) {
    const int tiles = ((Cout + kTile - 1) / kTile) * ((N + kTile - 1) / kTile);
    int S = (int)((256 + tiles - 1) / tiles);
    const int64_t by_len = (frames + 127) / 128;
    if (S > by_len) S = (int)by_len;
    if (S > kWgMaxSplits) S = kWgMaxSplits;
    if (S < 1) S = 1;
    int64_t f = (frames + S - 1) / S;
    f = (f + kWgChunk - 1) / kWgChunk * kWgChunk;
    *fs = (int)f;
    return (int)((frames + f - 1) / f);
}

inline size_t wgrad_scratch_floats(int64_t frames, int Cout, int N) {
    int fs = 0;
    const int S = wgrad_split(frames, Cout, N, &fs);
    return S > 1 ? (size_t)S * Cout * N : 0;
}

// out = planes[0] + planes[1] + ... + planes[S - 1], in that order (a template, as wgrad_kernel: emitted only where it is launched)
template <typename T>
__global__ __launch_bounds__(256) void sum_planes_kernel(const T* __restrict__ planes, T* __restrict__ out, int S, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        T v = planes[i];
        for (int s = 1; s < S; ++s) v += planes[(size_t)s * n + i];
        out[i] = v;
    }
}

// One plane: the kernel writes dw.  More: it writes the planes of `scratch` (wgrad_scratch_floats() floats), summed into dw.
template <typename Src>
hipError_t launch_wgrad(const Src& src, float* dw, float* scratch, hipStream_t st) {
    const int Cout = src.cout(), N = src.n();
    int fs = 0;
    const int S = wgrad_split(src.frames(), Cout, N, &fs);
    if (S > 1 && !scratch) return hipErrorInvalidValue;
    const dim3 grid((N + kTile - 1) / kTile, (Cout + kTile - 1) / kTile, S);
    hipLaunchKernelGGL(wgrad_kernel<Src>, grid, dim3(256), 0, st, src, fs, S > 1 ? scratch : dw);
    if (S > 1) {
        const int64_t n = (int64_t)Cout * N;
        hipLaunchKernelGGL(sum_planes_kernel<float>, dim3(grid_1d(n, 4096)), dim3(256), 0, st, scratch, dw, S, n);
    }
    return hipGetLastError();
}

}  // namespace st
