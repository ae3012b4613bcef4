// Resolution-discriminator kernels (vocoders/vocos/models/discriminator.py:112-171): the complex STFT and its backward on
// audio_fft.h's real FFT, the band convs ((3, 9) and (3, 3) taps, stride (1, 1) / (1, 2), 32 output channels) as implicit GEMMs
// on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fp32 FMA chain) with fp32_tile.h's 32 x 128 tile, their weight
// gradients on fp32_tile.h's split-K kernel, and layer 0's data gradient and conv_post as vector kernels.  fp32 throughout.
// No atomics anywhere: every reduction has a fixed order.  Layouts and formulas: resolution_disc_launch.h.
#include "audio_fft.h"
#include "audio_launch.h"
#include "fp32_tile.h"
#include "resolution_disc_launch.h"

namespace st {

// ---- complex STFT ------------------------------------------------------------------------------------------------------------
namespace {

// One block = FR consecutive frames of one item, S at a time (mel_kernel's tiling); Re and Im go straight to the conv layout.
template <int N>
__global__ __launch_bounds__(256) void rd_stft_kernel(const float* __restrict__ x, const float* __restrict__ win, float* __restrict__ spec,
                                                      int T, int frames, int tiles_per) {
    using G = MelGeo<N>;
    constexpr int H = G::H, S = G::S, FR = G::FR;
    __shared__ float2 buf[2][S * H];
    __shared__ float2 tw[H];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles_per, t0 = (blockIdx.x - b * tiles_per) * FR;
    const float* __restrict__ xb = x + (long long)b * T;
    float* __restrict__ re = spec + (long long)b * 2 * frames * (H + 1);
    float* __restrict__ im = re + (long long)frames * (H + 1);
    mel_twiddles<N>(tw, tid);
#pragma unroll 1
    for (int r = 0; r < FR / S; ++r) {
        const int tr = t0 + r * S;
        if (tr >= frames) break;                                              // block-uniform
        mel_frame_load<N>(reinterpret_cast<float*>(buf[0]), xb, win, tr, frames, N / 4, N / 2, T, tid);
        __syncthreads();
        const float2* Z = mel_fft<N>(buf[0], buf[1], tw, tid);
        for (int e = tid; e < S * (H + 1); e += 256) {
            const int f = e / (H + 1), k = e - f * (H + 1);
            const int t = tr + f;
            if (t < frames) {
                const float2 X = mel_split_bin<N>(Z, tw, f, k);
                re[(long long)t * (H + 1) + k] = X.x;
                im[(long long)t * (H + 1) + k] = X.y;
            }
        }
        __syncthreads();                                                       // buf is the next round's frame buffer
    }
}

// Per frame: C_k = (dRe_k + i dIm_k) / 2 (the two real bins: dRe_k, whose Im is identically zero in the forward), then the inverse
// real FFT, windowed, into the frame's row of ws.
template <int N>
__global__ __launch_bounds__(256) void rd_stft_bwd_kernel(const float* __restrict__ dspec, const float* __restrict__ win, float* __restrict__ ws,
                                                          int frames, int tiles_per) {
    using G = MelGeo<N>;
    constexpr int H = G::H, S = G::S, FR = G::FR;
    __shared__ float2 buf[2][S * H];
    __shared__ float2 tw[H];
    __shared__ float2 spec[S * (H + 1)];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles_per, t0 = (blockIdx.x - b * tiles_per) * FR;
    const float* __restrict__ dre = dspec + (long long)b * 2 * frames * (H + 1);
    const float* __restrict__ dim_ = dre + (long long)frames * (H + 1);
    float* __restrict__ wsb = ws + (long long)b * frames * N;
    mel_twiddles<N>(tw, tid);
#pragma unroll 1
    for (int r = 0; r < FR / S; ++r) {
        const int tr = t0 + r * S;
        if (tr >= frames) break;                                              // block-uniform
        for (int e = tid; e < S * (H + 1); e += 256) {
            const int f = e / (H + 1), k = e - f * (H + 1);
            const int t = tr + f;
            float2 g = make_float2(0.0f, 0.0f);
            if (t < frames) g = make_float2(dre[(long long)t * (H + 1) + k], dim_[(long long)t * (H + 1) + k]);
            spec[e] = (k == 0 || k == H) ? make_float2(g.x, 0.0f) : make_float2(0.5f * g.x, 0.5f * g.y);
        }
        __syncthreads();
        mel_inverse_to_ws<N>(spec, buf[0], buf[1], tw, wsb, win, tr, frames, tid);
        __syncthreads();                                                       // buf and spec are the next round's
    }
}

template <int N>
hipError_t rd_stft_n(const float* x, const float* win, float* spec, int B, int T, int frames, hipStream_t s) {
    const int tiles_per = (frames + MelGeo<N>::FR - 1) / MelGeo<N>::FR;
    hipLaunchKernelGGL((rd_stft_kernel<N>), dim3((unsigned)(B * tiles_per)), dim3(256), 0, s, x, win, spec, T, frames, tiles_per);
    return hipGetLastError();
}

template <int N>
hipError_t rd_stft_bwd_n(const float* dspec, const float* win, float* ws, int B, int frames, hipStream_t s) {
    const int tiles_per = (frames + MelGeo<N>::FR - 1) / MelGeo<N>::FR;
    hipLaunchKernelGGL((rd_stft_bwd_kernel<N>), dim3((unsigned)(B * tiles_per)), dim3(256), 0, s, dspec, win, ws, frames, tiles_per);
    return hipGetLastError();
}

bool rd_stft_ok(int W, int B, int T, int frames) {
    return W >= kMelMinNfft && W <= kMelMaxNfft && (W & (W - 1)) == 0 && B >= 1 && T > W / 2 && frames == 1 + T / (W / 4) &&
           (int64_t)B * frames < ((int64_t)1 << 30);
}

}  // namespace

hipError_t launch_rd_stft(const float* x, const float* window, float* spec, int W, int B, int T, int frames, hipStream_t s) {
    if (!x || !window || !spec || !rd_stft_ok(W, B, T, frames)) return hipErrorInvalidValue;
    switch (W) {
        case 32: return rd_stft_n<32>(x, window, spec, B, T, frames, s);
        case 64: return rd_stft_n<64>(x, window, spec, B, T, frames, s);
        case 128: return rd_stft_n<128>(x, window, spec, B, T, frames, s);
        case 256: return rd_stft_n<256>(x, window, spec, B, T, frames, s);
        case 512: return rd_stft_n<512>(x, window, spec, B, T, frames, s);
        case 1024: return rd_stft_n<1024>(x, window, spec, B, T, frames, s);
        case 2048: return rd_stft_n<2048>(x, window, spec, B, T, frames, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_rd_stft_backward(const float* dspec, const float* window, float* ws, float* dx, int W, int B, int T, int frames, hipStream_t s) {
    if (!dspec || !window || !ws || !dx || !rd_stft_ok(W, B, T, frames)) return hipErrorInvalidValue;
    hipError_t err;
    switch (W) {
        case 32: err = rd_stft_bwd_n<32>(dspec, window, ws, B, frames, s); break;
        case 64: err = rd_stft_bwd_n<64>(dspec, window, ws, B, frames, s); break;
        case 128: err = rd_stft_bwd_n<128>(dspec, window, ws, B, frames, s); break;
        case 256: err = rd_stft_bwd_n<256>(dspec, window, ws, B, frames, s); break;
        case 512: err = rd_stft_bwd_n<512>(dspec, window, ws, B, frames, s); break;
        case 1024: err = rd_stft_bwd_n<1024>(dspec, window, ws, B, frames, s); break;
        case 2048: err = rd_stft_bwd_n<2048>(dspec, window, ws, B, frames, s); break;
        default: return hipErrorInvalidValue;
    }
    if (err != hipSuccess) return err;
    MelBwdArgs g{};
    g.ws = ws; g.out = dx; g.n_fft = W; g.hop = W / 4; g.pad = W / 2; g.B = B; g.L = T; g.frames = frames;
    return launch_mel_gather(g, s);
}

// ---- band convs on the MFMA ----------------------------------------------------------------------------------------------------
enum RdMode { RD_FWD = 0, RD_DGRAD = 1 };

// Tiles of one launch: band c owns blockIdx.x in [tile0[c], tile0[c + 1]) and computes cols[c] columns of every frame row.  Forward:
// every output column.  Data gradient: the input columns fi = q + stride m, which take the taps jf = q + stride u only.
struct RdTiles { int tile0[kRdBands + 1]; int cols[kRdBands]; int q; };

// One block = 32 channels x 128 positions (t, column) of one item of one band on fp32_tile.h's 32 x 128 mapping.  K = (input channel,
// row tap, column tap) in the weight's order, CK channels x 3 x NU taps per LDS chunk.  TW: the column taps of the weight (9 / 3), NU:
// those this launch uses.  Xs is the im2col chunk [k][position]; a thread stages one position column (256 % 128 == 0), so the
// position -> (t, column) division happens once per thread.  Odd k rows are stored with their 32-column halves swapped: the two
// half-waves of an MFMA operand read (k, k + 1) land on disjoint banks.
template <int TW, int NU, int CK, int MODE>
__global__ __launch_bounds__(256) void rd_conv_kernel(RdConvArgs a, RdTiles tl) {
    constexpr int KC = CK * kRdRows * NU, WS = KC + 1, PW = TW / 2;
    static_assert(KC % 2 == 0, "the MFMA takes k in pairs");
    __shared__ float Ws[kWideRows * WS];
    __shared__ float Xs[KC * kWideCols];
    const int tid = threadIdx.x;
    const TileLane l = wide_lane();
    int c = 0;
    while (c + 1 < kRdBands && (int)blockIdx.x >= tl.tile0[c + 1]) ++c;
    const RdBand bd = a.band[c];
    const int b = blockIdx.z, Cin = a.Cin, Cout = a.Cout, Fr = a.frames, sw = a.stride_w, q = tl.q;
    const int cols = tl.cols[c], n0 = ((int)blockIdx.x - tl.tile0[c]) * kWideCols;
    // the position this thread stages
    const int fs = tid & (kWideCols - 1);
    const int ns = n0 + fs, ts = ns / cols, ms = ns - ts * cols;
    const bool s_ok = ts < Fr;
    // source row / column of taps (jt, u) = (0, 0) and the step between taps
    const int row0 = MODE == RD_FWD ? ts - 1 : ts + 1;
    const int col0 = MODE == RD_FWD ? sw * ms - PW : (sw == 2 ? ms + PW / 2 : ms + PW);
    const int dstep = MODE == RD_FWD ? 1 : -1;
    const float* inb = bd.in + (size_t)b * Cin * Fr * bd.in_rs;
    // Each channel chunk runs its own k-ordered chain from zero and the chunk sums are added in chunk order: the rounding error
    // grows with sqrt(KC) + sqrt(chunks) steps instead of sqrt(K) (K = 864 for the 32 -> 32 layers), at 16 adds per chunk and lane.
    f32x16 total = tile_zero();
    for (int ci0 = 0; ci0 < Cin; ci0 += CK) {
        f32x16 acc = tile_zero();
        if constexpr (MODE == RD_FWD) {
            static_assert(MODE != RD_FWD || NU == TW, "the forward uses every tap");
            for (int i = tid; i < kWideRows * KC; i += 256) {
                const int row = i / KC, kk = i - row * KC;
                const int ci = ci0 + kk / (kRdRows * NU);
                Ws[row * WS + kk] = (row < Cout && ci < Cin) ? bd.w[((size_t)row * Cin + ci0) * (kRdRows * TW) + kk] : 0.0f;
            }
        } else {
            // w[co_fwd = the K channel][ci_fwd = the output row][jt][jf = q + stride u]; the output row runs fastest across the lanes
            for (int i = tid; i < kWideRows * KC; i += 256) {
                const int kk = i / kWideRows, row = i - kk * kWideRows;
                const int cl = kk / (kRdRows * NU), r2 = kk - cl * (kRdRows * NU), jt = r2 / NU, u = r2 - jt * NU;
                const int cf = ci0 + cl;
                Ws[row * WS + kk] = (row < Cout && cf < Cin) ? bd.w[(((size_t)cf * Cout + row) * kRdRows + jt) * TW + q + sw * u] : 0.0f;
            }
        }
        for (int kk = tid >> 7; kk < KC; kk += 2) {
            const int cl = kk / (kRdRows * NU), r2 = kk - cl * (kRdRows * NU), jt = r2 / NU, u = r2 - jt * NU;
            const int ci = ci0 + cl, row = row0 + dstep * jt, col = col0 + dstep * u;
            float v = 0.0f;
            if (s_ok && ci < Cin && row >= 0 && row < Fr && col >= 0 && col < bd.Win) v = inb[((size_t)ci * Fr + row) * bd.in_rs + col];
            Xs[kk * kWideCols + (fs ^ ((kk & 1) << 5))] = v;
        }
        __syncthreads();
        tile_mfma<KC, 9>(acc, Ws, WS, l, [&](int k, int col) { return Xs[k * kWideCols + (col ^ ((k & 1) << 5))]; });
        __syncthreads();
        for (int i = 0; i < 16; ++i) total[i] += acc[i];
    }
    const int n = n0 + l.wt * 32 + l.r, t = n / cols, m = n - t * cols;
    if (t >= Fr) return;
    const int fo = MODE == RD_FWD ? m : q + sw * m;
    tile_for_each(total, l, [&](int row, float v) {
        if (row >= Cout) return;
        const size_t o = (((size_t)b * Cout + row) * Fr + t) * bd.Wout + fo;
        if constexpr (MODE == RD_FWD) {
            v += bd.bias[row];
            v = v > 0.0f ? v : v * a.slope;
            bd.out[o] = v;
            if (bd.out2) bd.out2[o] = v;
        } else {
            if (bd.addg) v += bd.addg[o];
            if (bd.act) v *= bd.act[o] > 0.0f ? 1.0f : a.slope;
            bd.out[o] = v;
        }
    });
}

static bool rd_conv_args_ok(const RdConvArgs& a, bool fwd) {
    if (a.B < 1 || a.B > 65535 || a.Cin < 1 || a.Cout < 1 || a.Cout > kWideRows || a.frames < 1) return false;
    if (!((a.taps_w == 9 && (a.stride_w == 1 || a.stride_w == 2)) || (a.taps_w == 3 && a.stride_w == 1))) return false;
    for (const RdBand& bd : a.band) {
        if (!bd.in || !bd.w || !bd.out || (fwd && !bd.bias) || bd.Win < 1 || bd.Wout < 1 || bd.in_rs < bd.Win) return false;
        const int wf_in = fwd ? bd.Win : bd.Wout, wf_out = fwd ? bd.Wout : bd.Win;      // the forward's widths
        if (wf_out != (wf_in - 1) / a.stride_w + 1) return false;
        if ((int64_t)a.frames * (bd.in_rs > bd.Wout ? bd.in_rs : bd.Wout) >= ((int64_t)1 << 30)) return false;
    }
    return true;
}

// tiles of the columns fi = q + stride m < Wout of every band
static RdTiles rd_tiles(const RdConvArgs& a, int q, int stride) {
    RdTiles tl{};
    tl.q = q;
    for (int c = 0; c < kRdBands; ++c) {
        const int W = a.band[c].Wout;
        tl.cols[c] = q < W ? (W - 1 - q) / stride + 1 : 0;
        tl.tile0[c + 1] = tl.tile0[c] + (int)(((int64_t)a.frames * tl.cols[c] + kWideCols - 1) / kWideCols);
        if (tl.cols[c] == 0) tl.cols[c] = 1;      // no tile of this band runs; keeps the kernel's divisor valid
    }
    return tl;
}

template <int TW, int NU, int CK, int MODE>
static hipError_t rd_conv_launch(const RdConvArgs& a, const RdTiles& tl, hipStream_t s) {
    if (tl.tile0[kRdBands] > 0)
        hipLaunchKernelGGL((rd_conv_kernel<TW, NU, CK, MODE>), dim3(tl.tile0[kRdBands], 1, a.B), dim3(256), 0, s, a, tl);
    return hipGetLastError();
}

hipError_t launch_rd_conv(const RdConvArgs& a, hipStream_t s) {
    if (!rd_conv_args_ok(a, true)) return hipErrorInvalidValue;
    const RdTiles tl = rd_tiles(a, 0, 1);
    return a.taps_w == 9 ? rd_conv_launch<9, 9, 2, RD_FWD>(a, tl, s) : rd_conv_launch<3, 3, 4, RD_FWD>(a, tl, s);
}

hipError_t launch_rd_conv_dgrad(const RdConvArgs& a, hipStream_t s) {
    if (!rd_conv_args_ok(a, false)) return hipErrorInvalidValue;
    if (a.taps_w == 3) return rd_conv_launch<3, 3, 4, RD_DGRAD>(a, rd_tiles(a, 0, 1), s);
    if (a.stride_w != 2) return hipErrorInvalidValue;       // (3, 9) taps with stride 1 is layer 0: launch_rd_l0_dgrad
    hipError_t err = rd_conv_launch<9, 5, 4, RD_DGRAD>(a, rd_tiles(a, 0, 2), s);      // even columns: taps 0, 2, 4, 6, 8
    if (err != hipSuccess) return err;
    return rd_conv_launch<9, 4, 4, RD_DGRAD>(a, rd_tiles(a, 1, 2), s);                // odd columns: taps 1, 3, 5, 7
}

// ---- weight gradient: dW[co][n] = sum_f dY[f][co] X'[f][n], n = (ci, jt, jf), f = (b, t, column) -----------------------------------
struct RdWgradSrc {
    RdWgradArgs a;
    struct Frame { int b, t, f; };
    __host__ __device__ int cout() const { return kRdCh; }
    __host__ __device__ int n() const { return a.Cin * kRdRows * a.taps_w; }
    __host__ __device__ int No() const { return a.frames * a.Wout; }      // positions of one item
    __host__ __device__ int64_t frames() const { return (int64_t)a.B * No(); }
    __device__ Frame frame(int64_t f) const {
        const int b = (int)(f / No()), nf = (int)(f - (int64_t)b * No()), t = nf / a.Wout;
        return {b, t, nf - t * a.Wout};
    }
    __device__ float dy(Frame f, int co) const { return a.dy[(((size_t)f.b * kRdCh + co) * a.frames + f.t) * a.Wout + f.f]; }
    __device__ float x(Frame f, int nn) const {
        const int kt = kRdRows * a.taps_w, ci = nn / kt, r2 = nn - ci * kt, jt = r2 / a.taps_w, jf = r2 - jt * a.taps_w;
        const int row = f.t + jt - 1, col = a.stride_w * f.f + jf - a.taps_w / 2;
        return row >= 0 && row < a.frames && col >= 0 && col < a.Win ? a.in[(((size_t)f.b * a.Cin + ci) * a.frames + row) * a.in_rs + col] : 0.0f;
    }
};

int rd_wgrad_planes(int B, int Cin, int frames, int Wout, int taps_w) {
    int fs = 0;
    return wgrad_split((int64_t)B * frames * Wout, kRdCh, Cin * kRdRows * taps_w, &fs);
}

size_t rd_wgrad_scratch_floats(int B, int Cin, int frames, int Wout, int taps_w) {
    return wgrad_scratch_floats((int64_t)B * frames * Wout, kRdCh, Cin * kRdRows * taps_w);
}

hipError_t launch_rd_wgrad(const RdWgradArgs& a, hipStream_t st) {
    if (a.B < 1 || a.Cin < 1 || a.frames < 1 || a.Win < 1 || a.Wout < 1 || a.in_rs < a.Win || !a.dy || !a.in || !a.dw) return hipErrorInvalidValue;
    if (!((a.taps_w == 9 && (a.stride_w == 1 || a.stride_w == 2)) || (a.taps_w == 3 && a.stride_w == 1))) return hipErrorInvalidValue;
    if (a.Wout != (a.Win - 1) / a.stride_w + 1 || (int64_t)a.frames * a.in_rs >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
    return launch_wgrad(RdWgradSrc{a}, a.dw, a.scratch, st);
}

// ---- layer 0's data gradient ---------------------------------------------------------------------------------------------------
// One thread = one bin (t, k) of one spectrum channel (blockIdx.y) of one item (blockIdx.z): the bands that hold k in order, and per
// band the 32 channels in order, each the sum of its 27 taps in the weight's order.  The weight index is uniform but for the band: the loads broadcast.
__global__ __launch_bounds__(256) void rd_l0_dgrad_kernel(RdL0DgradArgs a) {
    const int Fr = a.frames, NB = a.bins, ch = blockIdx.y, b = blockIdx.z;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Fr * NB) return;
    const int t = n / NB, k = n - t * NB;
    float v = 0.0f;
#pragma unroll
    for (int c = 0; c < kRdBands; ++c) {
        const int lo = a.lo[c], Wb = a.hi[c] - lo;
        if (k < lo || k >= lo + Wb) continue;
        const float* __restrict__ d0 = a.d0[c] + (size_t)b * kRdCh * Fr * Wb;
        const float* __restrict__ w = a.w[c] + ch * (kRdRows * 9);
        const int f = k - lo;
        for (int co = 0; co < kRdCh; ++co) {
            float p = 0.0f;       // the channel's 27 taps, then the channels in order: shorter rounding chains than one of 864
#pragma unroll
            for (int jt = 0; jt < kRdRows; ++jt) {
                const int row = t + 1 - jt;
                if (row < 0 || row >= Fr) continue;
                const float* __restrict__ dr = d0 + ((size_t)co * Fr + row) * Wb;
#pragma unroll
                for (int jf = 0; jf < 9; ++jf) {
                    const int col = f + 4 - jf;
                    if (col >= 0 && col < Wb) p = fmaf(w[(co * 2) * (kRdRows * 9) + jt * 9 + jf], dr[col], p);
                }
            }
            v += p;
        }
    }
    a.dspec[(((size_t)b * 2 + ch) * Fr + t) * NB + k] = v;
}

hipError_t launch_rd_l0_dgrad(const RdL0DgradArgs& a, hipStream_t s) {
    if (!a.dspec || a.B < 1 || a.B > 65535 || a.frames < 1 || a.bins < 1 || (int64_t)a.frames * a.bins >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
    for (int c = 0; c < kRdBands; ++c)
        if (!a.d0[c] || !a.w[c] || a.lo[c] < 0 || a.hi[c] <= a.lo[c] || a.hi[c] > a.bins) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rd_l0_dgrad_kernel, dim3((a.frames * a.bins + 255) / 256, 2, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- conv_post -----------------------------------------------------------------------------------------------------------------
// column fc of the concatenation -> its band's tensor, row width and column there; ok: fc inside [0, Wc)
struct RdCatCol { const float* in; int width, col; bool ok; };
__device__ __forceinline__ RdCatCol rd_cat_col(const RdPostArgs& a, int fc) {
    RdCatCol r{a.in[0], a.off[1], fc, fc >= 0 && fc < a.off[kRdBands]};
#pragma unroll
    for (int i = 1; i < kRdBands; ++i)
        if (fc >= a.off[i]) { r.in = a.in[i]; r.width = a.off[i + 1] - a.off[i]; r.col = fc - a.off[i]; }
    return r;
}

// One thread = one output (t, fc) of one item: the 32 channels in order, each the sum of its 9 taps in the weight's order.
__global__ __launch_bounds__(256) void rd_post_fwd_kernel(RdPostArgs a) {
    const int Fr = a.frames, Wc = a.off[kRdBands], b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Fr * Wc) return;
    const int t = n / Wc, fc = n - t * Wc;
    const float* base[3]; int width[3]; bool okc[3];
#pragma unroll
    for (int jf = 0; jf < 3; ++jf) {
        const RdCatCol cc = rd_cat_col(a, fc + jf - 1);
        okc[jf] = cc.ok;
        width[jf] = cc.width;
        base[jf] = cc.in + (size_t)b * kRdCh * Fr * cc.width + cc.col;
    }
    float v = 0.0f;
    for (int ci = 0; ci < kRdCh; ++ci) {
        float p = 0.0f;
#pragma unroll
        for (int jt = 0; jt < kRdRows; ++jt) {
            const int row = t + jt - 1;
            if (row < 0 || row >= Fr) continue;
#pragma unroll
            for (int jf = 0; jf < 3; ++jf)
                if (okc[jf]) p = fmaf(a.w[ci * 9 + jt * 3 + jf], base[jf][((size_t)ci * Fr + row) * width[jf]], p);
        }
        v += p;
    }
    v += a.bias[0];
    a.out[(size_t)b * Fr * Wc + n] = v;
    if (a.out2) a.out2[(size_t)b * Fr * Wc + n] = v;
}

static bool rd_post_ok(const RdPostArgs& a) {
    if (a.B < 1 || a.B > 65535 || a.frames < 1 || !a.w || a.off[0] != 0) return false;
    for (int c = 0; c < kRdBands; ++c) if (!a.in[c] || a.off[c + 1] <= a.off[c]) return false;
    return (int64_t)a.frames * a.off[kRdBands] < ((int64_t)1 << 30);
}

hipError_t launch_rd_post_fwd(const RdPostArgs& a, hipStream_t s) {
    if (!rd_post_ok(a) || !a.bias || !a.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rd_post_fwd_kernel, dim3((a.frames * a.off[kRdBands] + 255) / 256, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// blockIdx.y = the band; a grid-stride loop over its (B, 32, frames, width) elements
__global__ __launch_bounds__(256) void rd_post_dgrad_kernel(RdPostArgs a) {
    const int c = blockIdx.y, Fr = a.frames, Wc = a.off[kRdBands], o0 = a.off[c], Wb = a.off[c + 1] - o0;
    const float* __restrict__ act = a.in[c];
    const float* __restrict__ addg = a.addg[c];
    float* __restrict__ dpre = a.dpre[c];
    const int64_t total = (int64_t)a.B * kRdCh * Fr * Wb;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / Wb;
        const int f = (int)(i - r * Wb);
        const int64_t bc = r / Fr;
        const int t = (int)(r - bc * Fr);
        const int64_t b = bc / kRdCh;
        const int ci = (int)(bc - b * kRdCh);
        float v = 0.0f;
        if (a.dy) {
            const float* __restrict__ dyb = a.dy + (size_t)b * Fr * Wc;
#pragma unroll
            for (int jt = 0; jt < kRdRows; ++jt) {
                const int row = t + 1 - jt;
                if (row < 0 || row >= Fr) continue;
#pragma unroll
                for (int jf = 0; jf < 3; ++jf) {
                    const int col = o0 + f + 1 - jf;
                    if (col >= 0 && col < Wc) v = fmaf(a.w[ci * 9 + jt * 3 + jf], dyb[(size_t)row * Wc + col], v);
                }
            }
        }
        if (addg) v += addg[i];
        dpre[i] = v * (act[i] > 0.0f ? 1.0f : a.slope);
    }
}

hipError_t launch_rd_post_dgrad(const RdPostArgs& a, hipStream_t s) {
    if (!rd_post_ok(a)) return hipErrorInvalidValue;
    int64_t most = 0;
    for (int c = 0; c < kRdBands; ++c) {
        if (!a.dpre[c]) return hipErrorInvalidValue;
        const int64_t n = (int64_t)a.B * kRdCh * a.frames * (a.off[c + 1] - a.off[c]);
        most = n > most ? n : most;
    }
    hipLaunchKernelGGL(rd_post_dgrad_kernel, dim3(grid_1d(most, 4096), kRdBands), dim3(256), 0, s, a);
    return hipGetLastError();
}

// Position ranges of the O(N) reductions below: ranges of kRdRangeLen positions, at most kRdMaxRanges (fixed by the shape alone)
constexpr int kRdRangeLen = 8192, kRdMaxRanges = 64;
static int rd_ranges(int64_t positions) {
    const int64_t S = (positions + kRdRangeLen - 1) / kRdRangeLen;
    return (int)(S < 1 ? 1 : (S > kRdMaxRanges ? kRdMaxRanges : S));
}

// Block (channel, range): its range of the (item, t, fc) positions in strides of 256, a fixed LDS tree -> part[range][channel][9]
__global__ __launch_bounds__(256) void rd_post_wgrad_kernel(RdPostArgs a, int len) {
    __shared__ float red[9][256];
    const int ci = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, Fr = a.frames, Wc = a.off[kRdBands], No = Fr * Wc;
    const int F = a.B * No, lo = r * len, hi = lo + len < F ? lo + len : F;
    float acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = 0.0f;
    for (int p = lo + tid; p < hi; p += 256) {
        const int b = p / No, n = p - b * No;
        const int t = n / Wc, fc = n - t * Wc;
        const float g = a.dy[p];
#pragma unroll
        for (int jf = 0; jf < 3; ++jf) {
            const RdCatCol cc = rd_cat_col(a, fc + jf - 1);
            if (!cc.ok) continue;
            const float* __restrict__ ib = cc.in + (((size_t)b * kRdCh + ci) * Fr) * cc.width + cc.col;
#pragma unroll
            for (int jt = 0; jt < kRdRows; ++jt) {
                const int row = t + jt - 1;
                if (row >= 0 && row < Fr) acc[jt * 3 + jf] = fmaf(g, ib[(size_t)row * cc.width], acc[jt * 3 + jf]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) red[j][tid] = acc[j];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int j = 0; j < 9; ++j) red[j][tid] += red[j][tid + w];
        }
        __syncthreads();
    }
    if (tid < 9) a.part[((size_t)r * kRdCh + ci) * 9 + tid] = red[tid][0];
}

// out[i] = part[0][i] + part[1][i] + ... in range order, i < n (n <= 1024: one block)
__global__ __launch_bounds__(256) void rd_sum_ranges_kernel(const float* __restrict__ part, float* __restrict__ out, int S, int n) {
    for (int i = threadIdx.x; i < n; i += 256) {
        float v = part[i];
        for (int r = 1; r < S; ++r) v += part[(size_t)r * n + i];
        out[i] = v;
    }
}

size_t rd_post_wgrad_scratch_floats(int B, int frames, int Wc) { return (size_t)rd_ranges((int64_t)B * frames * Wc) * kRdCh * 9; }

hipError_t launch_rd_post_wgrad(const RdPostArgs& a, hipStream_t s) {
    if (!rd_post_ok(a) || !a.dy || !a.dw || !a.part) return hipErrorInvalidValue;
    const int64_t F = (int64_t)a.B * a.frames * a.off[kRdBands];
    if (F >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int S = rd_ranges(F), len = (int)((F + S - 1) / S);
    hipLaunchKernelGGL(rd_post_wgrad_kernel, dim3(kRdCh, S), dim3(256), 0, s, a, len);
    hipLaunchKernelGGL(rd_sum_ranges_kernel, dim3(1), dim3(256), 0, s, a.part, a.dw, S, kRdCh * 9);
    return hipGetLastError();
}

// ---- bias gradients ------------------------------------------------------------------------------------------------------------
// Block (channel, band, range): the band's positions (item, t, f) of its range in strides of 256, a fixed LDS tree -> part[band][range][channel]
__global__ __launch_bounds__(256) void rd_bias_grad_kernel(RdBiasArgs a, int S) {
    __shared__ float red[256];
    const int co = blockIdx.x, c = blockIdx.y, r = blockIdx.z, No = a.frames * a.width[c];
    const int F = a.B * No, len = (F + S - 1) / S, lo = r * len, hi = lo + len < F ? lo + len : F;
    const float* __restrict__ d = a.d[c];
    float v = 0.0f;
    for (int p = lo + (int)threadIdx.x; p < hi; p += 256) {
        const int b = p / No, n = p - b * No;
        v += d[((size_t)b * kRdCh + co) * No + n];
    }
    v = block_sum256(red, v);
    if (threadIdx.x == 0) a.part[((size_t)c * S + r) * kRdCh + co] = v;
}

__global__ __launch_bounds__(256) void rd_bias_sum_kernel(RdBiasArgs a, int S) {
    const int i = threadIdx.x;
    if (i >= kRdBands * kRdCh) return;
    const int c = i / kRdCh, co = i - c * kRdCh;
    float v = a.part[((size_t)c * S) * kRdCh + co];
    for (int r = 1; r < S; ++r) v += a.part[((size_t)c * S + r) * kRdCh + co];
    float* dst = a.db[0];
#pragma unroll
    for (int k = 1; k < kRdBands; ++k) dst = k == c ? a.db[k] : dst;
    dst[co] = v;
}

size_t rd_bias_scratch_floats(int B, int frames, int widest) { return (size_t)kRdBands * rd_ranges((int64_t)B * frames * widest) * kRdCh; }

hipError_t launch_rd_bias_grad(const RdBiasArgs& a, hipStream_t s) {
    if (a.B < 1 || a.frames < 1 || !a.part) return hipErrorInvalidValue;
    int widest = 0;
    for (int c = 0; c < kRdBands; ++c) {
        if (!a.d[c] || !a.db[c] || a.width[c] < 1) return hipErrorInvalidValue;
        widest = a.width[c] > widest ? a.width[c] : widest;
    }
    if ((int64_t)a.B * a.frames * widest >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int S = rd_ranges((int64_t)a.B * a.frames * widest);      // the widest band's: a narrower band's ranges are shorter
    hipLaunchKernelGGL(rd_bias_grad_kernel, dim3(kRdCh, kRdBands, S), dim3(256), 0, s, a, S);
    hipLaunchKernelGGL(rd_bias_sum_kernel, dim3(1), dim3(256), 0, s, a, S);
    return hipGetLastError();
}

}  // namespace st
