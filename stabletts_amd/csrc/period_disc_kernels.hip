// Period-discriminator kernels (vocoders/vocos/models/discriminator.py:32-75): forward, data gradient and weight gradient of the
// (5, 1) convs with stride (3, 1) / (1, 1) on (B, C, H, p) tensors, layer 0 with the reflect tail padding, conv_post and the
// weight norm.  fp32 throughout.  Layers 1-4 are GEMMs (M = Cout, K = Cin x taps, N = B Hout p) on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: a k-ordered fp32 FMA chain) on the 64 x 64 tile of fp32_tile.h, which sd_conv_kernel
// (style_dp_kernels.hip) shares; the operand staging is this file's own: it gathers the strided rows of the period view into an
// im2col chunk in LDS.  No atomics anywhere: every reduction has a fixed order.
#include "fp32_tile.h"
#include "period_disc_launch.h"

#include <math.h>

namespace st {

enum PdMode { PD_FWD = 0, PD_DGRAD = 1 };

// Tile families of one launch: family c owns blockIdx.x in [tile0[c], tile0[c + 1]).  Forward: one family.  Data gradient: one
// per residue class q = (hi + 2) % stride of the input rows; its rows are hi = hi0 + stride m and its taps j = q + stride u.
struct PdFamilies { int n = 0; int tile0[4] = {0, 0, 0, 0}; int q[3] = {0, 0, 0}; int hi0[3] = {0, 0, 0}; int rows[3] = {0, 0, 0}; };

// One block = a 64 (channel) x 64 (frame) output tile of one item on fp32_tile.h's wave / lane mapping.  K = (input channel, tap)
// pairs, 16 channels x NT taps per LDS chunk, in the weight's own order.  Xs is the im2col chunk [k][frame]: a thread stages one
// frame column (256 % 64 == 0), so the frame -> (row, w) division happens once per thread.
template <int NT, int MODE>
__global__ __launch_bounds__(256) void pd_conv_kernel(PdConvArgs a, PdFamilies fam) {
    constexpr int KC = kTileChunk * NT, WS = KC + 1;
    __shared__ float Ws[kTile * WS];
    __shared__ float Xs[KC * kTile];
    const int tid = threadIdx.x;
    const TileLane l = tile_lane();
    const int co0 = blockIdx.y * kTile, b = blockIdx.z;
    const int Cin = a.Cin, Cout = a.Cout, Hin = a.Hin, Hout = a.Hout, p = a.p, st = a.stride;
    int c = 0;
    while (c + 1 < fam.n && (int)blockIdx.x >= fam.tile0[c + 1]) ++c;
    const int q = fam.q[c], n0 = ((int)blockIdx.x - fam.tile0[c]) * kTile;
    const int rows = MODE == PD_FWD ? Hout : fam.rows[c];         // rows of this family, p frames each
    // the frame this thread stages: output row (forward) / input-gradient row of the family (data gradient)
    const int fs = tid & 63;
    const int ns = n0 + fs, ms = ns / p, wsx = ns - ms * p;
    const bool s_ok = ms < rows;
    // first source row of tap u = 0 and the step between taps
    const int src0 = MODE == PD_FWD ? st * ms - kPdTaps / 2 : (fam.hi0[c] + st * ms + kPdTaps / 2 - q) / st;
    const int dsrc = MODE == PD_FWD ? 1 : -1;
    const float* inb = a.in + (size_t)b * Cin * Hin * p;
    f32x16 acc = tile_zero();
    for (int ci0 = 0; ci0 < Cin; ci0 += kTileChunk) {
        if constexpr (MODE == PD_FWD) {
            for (int i = tid; i < kTile * KC; i += 256) {
                const int row = i / KC, kk = i - row * KC;
                const int co = co0 + row, ci = ci0 + kk / NT;
                Ws[row * WS + kk] = (co < Cout && ci < Cin) ? a.w[((size_t)co * Cin + ci0) * kPdTaps + kk] : 0.0f;
            }
        } else {
            // w[co_fwd = ci][ci_fwd = co][j], j = q + stride u; the output channel runs fastest across the lanes
            for (int i = tid; i < kTile * KC; i += 256) {
                const int kk = i / kTile, row = i - kk * kTile;
                const int cl = kk / NT, u = kk - cl * NT;
                const int co = co0 + row, ci = ci0 + cl;
                Ws[row * WS + kk] = (co < Cout && ci < Cin) ? a.w[((size_t)ci * Cout + co) * kPdTaps + q + st * u] : 0.0f;
            }
        }
        for (int kk = tid >> 6; kk < KC; kk += 4) {
            const int cl = kk / NT, u = kk - cl * NT;
            const int ci = ci0 + cl, src = src0 + dsrc * u;
            float v = 0.0f;
            if (s_ok && ci < Cin && src >= 0 && src < Hin) v = inb[((size_t)ci * Hin + src) * p + wsx];
            Xs[kk * kTile + fs] = v;
        }
        __syncthreads();
        tile_mfma<KC, 8>(acc, Ws, WS, l, [&](int k, int col) { return Xs[k * kTile + col]; });
        __syncthreads();
    }
    const int n = n0 + l.wt * 32 + l.r, m = n / p, w = n - m * p;
    if (m >= rows) return;
    const int orow = MODE == PD_FWD ? m : fam.hi0[c] + st * m;
    tile_for_each(acc, l, [&](int row, float v) {
        const int co = co0 + row;
        if (co >= Cout) return;
        const size_t o = (((size_t)b * Cout + co) * Hout + orow) * p + w;
        if constexpr (MODE == PD_FWD) {
            v += a.bias[co];
            v = v > 0.0f ? v : v * a.slope;
            a.out[o] = v;
            if (a.out2) a.out2[o] = v;
        } else {
            if (a.addg) v += a.addg[o];
            if (a.act) v *= a.act[o] > 0.0f ? 1.0f : a.slope;
            a.out[o] = v;
        }
    });
}

static bool pd_conv_args_ok(const PdConvArgs& a) {
    return a.B >= 1 && a.B <= 65535 && a.Cin >= 1 && a.Cout >= 1 && a.Hin >= 1 && a.Hout >= 1 && a.p >= 1 && (a.stride == 1 || a.stride == 3) &&
           a.in && a.w && a.out && (int64_t)a.Hin * a.p < ((int64_t)1 << 30) && (int64_t)a.Hout * a.p < ((int64_t)1 << 30);
}

hipError_t launch_pd_conv(const PdConvArgs& a, hipStream_t s) {
    if (!pd_conv_args_ok(a) || !a.bias) return hipErrorInvalidValue;
    if (a.Hout != (a.Hin - 1) / a.stride + 1) return hipErrorInvalidValue;
    PdFamilies fam;
    fam.n = 1;
    fam.tile0[1] = (a.Hout * a.p + kTile - 1) / kTile;
    const dim3 grid(fam.tile0[1], (a.Cout + kTile - 1) / kTile, a.B), blk(256);
    hipLaunchKernelGGL((pd_conv_kernel<kPdTaps, PD_FWD>), grid, blk, 0, s, a, fam);
    return hipGetLastError();
}

hipError_t launch_pd_conv_dgrad(const PdConvArgs& a, hipStream_t s) {
    if (!pd_conv_args_ok(a)) return hipErrorInvalidValue;
    if (a.Hin != (a.Hout - 1) / a.stride + 1) return hipErrorInvalidValue;       // a.Hin = the forward's output rows
    const int st = a.stride, cy = (a.Cout + kTile - 1) / kTile;
    if (st == 1) {
        PdFamilies fam;
        fam.n = 1; fam.rows[0] = a.Hout;
        fam.tile0[1] = (a.Hout * a.p + kTile - 1) / kTile;
        hipLaunchKernelGGL((pd_conv_kernel<kPdTaps, PD_DGRAD>), dim3(fam.tile0[1], cy, a.B), dim3(256), 0, s, a, fam);
        return hipGetLastError();
    }
    // stride 3: rows with (hi + 2) % 3 == 0 / 1 take taps {0, 3} / {1, 4} (two-tap tiles), rows with == 2 take tap 2 alone
    PdFamilies two, one;
    for (int q = 0; q < 3; ++q) {
        const int hi0 = (q + st - 2) % st;
        const int rows = hi0 < a.Hout ? (a.Hout - 1 - hi0) / st + 1 : 0;
        PdFamilies& f = q < 2 ? two : one;
        const int k = f.n++;
        f.q[k] = q; f.hi0[k] = hi0; f.rows[k] = rows;
        f.tile0[k + 1] = f.tile0[k] + (rows * a.p + kTile - 1) / kTile;
    }
    if (two.tile0[two.n] > 0) hipLaunchKernelGGL((pd_conv_kernel<2, PD_DGRAD>), dim3(two.tile0[two.n], cy, a.B), dim3(256), 0, s, a, two);
    if (one.tile0[one.n] > 0) hipLaunchKernelGGL((pd_conv_kernel<1, PD_DGRAD>), dim3(one.tile0[one.n], cy, a.B), dim3(256), 0, s, a, one);
    return hipGetLastError();
}

// ---- weight gradient: dW[co][n] = sum_f dY[f][co] X'[f][n], n = ci * 5 + j, f = (b, h, w) --------------------------------
// fp32_tile.h's split-K kernel on the frames (b, h, w) of the period view; X' gathers the strided rows, zero outside [0, Hin).
struct PdWgradSrc {
    PdWgradArgs a;
    struct Frame { int b, n, h, w; };
    __host__ __device__ int cout() const { return a.Cout; }
    __host__ __device__ int n() const { return a.Cin * kPdTaps; }
    __host__ __device__ int No() const { return a.Hout * a.p; }      // frames of one item
    __host__ __device__ int64_t frames() const { return (int64_t)a.B * No(); }
    __device__ Frame frame(int64_t f) const {
        const int b = (int)(f / No()), nf = (int)(f - (int64_t)b * No()), h = nf / a.p;
        return {b, nf, h, nf - h * a.p};
    }
    __device__ float dy(Frame f, int co) const { return a.dy[((size_t)f.b * a.Cout + co) * No() + f.n]; }
    __device__ float x(Frame f, int nn) const {
        const int ci = nn / kPdTaps, src = a.stride * f.h + (nn - ci * kPdTaps) - kPdTaps / 2;
        return src >= 0 && src < a.Hin ? a.in[(((size_t)f.b * a.Cin + ci) * a.Hin + src) * a.p + f.w] : 0.0f;
    }
};

int pd_wgrad_planes(int B, int Cin, int Cout, int Hout, int p) {
    int fs = 0;
    return wgrad_split((int64_t)B * Hout * p, Cout, Cin * kPdTaps, &fs);
}

size_t pd_wgrad_scratch_floats(int B, int Cin, int Cout, int Hout, int p) { return wgrad_scratch_floats((int64_t)B * Hout * p, Cout, Cin * kPdTaps); }

hipError_t launch_pd_wgrad(const PdWgradArgs& a, hipStream_t st) {
    if (a.B < 1 || a.Cin < 1 || a.Cout < 1 || a.Hin < 1 || a.Hout < 1 || a.p < 1 || (a.stride != 1 && a.stride != 3) || !a.dy || !a.in || !a.dw)
        return hipErrorInvalidValue;
    if (a.Hout != (a.Hin - 1) / a.stride + 1 || (int64_t)a.Hout * a.p >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
    return launch_wgrad(PdWgradSrc{a}, a.dw, a.scratch, st);
}

// ---- layer 0 ---------------------------------------------------------------------------------------------------------------
// sample n of the padded waveform of one item (n < Tp, Tp - T < T)
__device__ __forceinline__ float pd_xpad(const float* __restrict__ xb, int n, int T) { return xb[n < T ? n : 2 * (T - 1) - n]; }

// One thread = one output frame (h, w) of one item, all 32 channels: five waveform samples in registers, the weights in LDS.
__global__ __launch_bounds__(256) void pd_l0_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ out, int T, int Tp, int H0, int p, float slope) {
    __shared__ float wsm[kPdC0 * kPdTaps + kPdC0];
    if (threadIdx.x < kPdC0 * kPdTaps) wsm[threadIdx.x] = w[threadIdx.x];
    else if (threadIdx.x < kPdC0 * kPdTaps + kPdC0) wsm[threadIdx.x] = bias[threadIdx.x - kPdC0 * kPdTaps];
    __syncthreads();
    const int b = blockIdx.y, No = H0 * p, Hp = Tp / p;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= No) return;
    const int h = n / p, wv = n - h * p;
    const float* xb = x + (size_t)b * T;
    float xv[kPdTaps];
#pragma unroll
    for (int j = 0; j < kPdTaps; ++j) {
        const int src = 3 * h + j - kPdTaps / 2;
        xv[j] = src >= 0 && src < Hp ? pd_xpad(xb, src * p + wv, T) : 0.0f;
    }
    float* ob = out + (size_t)b * kPdC0 * No + n;
    for (int co = 0; co < kPdC0; ++co) {
        float v = 0.0f;
#pragma unroll
        for (int j = 0; j < kPdTaps; ++j) v = fmaf(wsm[co * kPdTaps + j], xv[j], v);
        v += wsm[kPdC0 * kPdTaps + co];
        ob[(size_t)co * No] = v > 0.0f ? v : v * slope;
    }
}

hipError_t launch_pd_l0_fwd(const float* x, const float* w, const float* bias, float* out, int B, int T, int Tp, int H0, int p, float slope,
                            hipStream_t s) {
    if (!x || !w || !bias || !out || B < 1 || B > 65535 || T < 1 || p < 1 || Tp < T || Tp % p != 0 || Tp - T >= T || H0 != (Tp / p - 1) / 3 + 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pd_l0_fwd_kernel, dim3((H0 * p + 255) / 256, B), dim3(256), 0, s, x, w, bias, out, T, Tp, H0, p, slope);
    return hipGetLastError();
}

// dw / db partial sums: block (co, split) walks its frame range of (b, h, w) in strides of 256, a fixed LDS tree adds the lanes.
constexpr int kPdL0MaxSplits = 64, kPdL0SplitFrames = 4096;

static int pd_l0_splits(int64_t frames) {
    int64_t S = (frames + kPdL0SplitFrames - 1) / kPdL0SplitFrames;
    return (int)(S < 1 ? 1 : (S > kPdL0MaxSplits ? kPdL0MaxSplits : S));
}

size_t pd_l0_scratch_floats(int B, int H0, int p) { return (size_t)pd_l0_splits((int64_t)B * H0 * p) * kPdC0 * (kPdTaps + 1); }

__global__ __launch_bounds__(256) void pd_l0_wgrad_kernel(const float* __restrict__ dpre, const float* __restrict__ x, float* __restrict__ part,
                                                          int B, int T, int Tp, int H0, int p, int64_t fs) {
    __shared__ float red[kPdTaps + 1][256];
    const int co = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, No = H0 * p, Hp = Tp / p;
    const int64_t F = (int64_t)B * No, f_lo = (int64_t)s * fs, f_hi = f_lo + fs < F ? f_lo + fs : F;
    float acc[kPdTaps + 1];
#pragma unroll
    for (int j = 0; j <= kPdTaps; ++j) acc[j] = 0.0f;
    for (int64_t f = f_lo + tid; f < f_hi; f += 256) {
        const int b = (int)(f / No), n = (int)(f - (int64_t)b * No);
        const int h = n / p, wv = n - h * p;
        const float g = dpre[((size_t)b * kPdC0 + co) * No + n];
        const float* xb = x + (size_t)b * T;
#pragma unroll
        for (int j = 0; j < kPdTaps; ++j) {
            const int src = 3 * h + j - kPdTaps / 2;
            if (src >= 0 && src < Hp) acc[j] = fmaf(g, pd_xpad(xb, src * p + wv, T), acc[j]);
        }
        acc[kPdTaps] += g;
    }
#pragma unroll
    for (int j = 0; j <= kPdTaps; ++j) red[j][tid] = acc[j];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int j = 0; j <= kPdTaps; ++j) red[j][tid] += red[j][tid + w];
        }
        __syncthreads();
    }
    if (tid <= kPdTaps) part[((size_t)s * kPdC0 + co) * (kPdTaps + 1) + tid] = red[tid][0];
}

__global__ __launch_bounds__(256) void pd_l0_wgrad_sum_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int S) {
    const int i = threadIdx.x;
    if (i >= kPdC0 * (kPdTaps + 1)) return;
    float v = part[i];
    for (int s = 1; s < S; ++s) v += part[(size_t)s * kPdC0 * (kPdTaps + 1) + i];
    const int co = i / (kPdTaps + 1), j = i - co * (kPdTaps + 1);
    if (j < kPdTaps) dw[co * kPdTaps + j] = v; else db[co] = v;
}

hipError_t launch_pd_l0_wgrad(const float* dpre, const float* x, float* dw, float* db, float* scratch, int B, int T, int Tp, int H0, int p,
                              hipStream_t s) {
    if (!dpre || !x || !dw || !db || !scratch || B < 1 || T < 1 || p < 1 || Tp < T || Tp % p != 0 || Tp - T >= T || H0 != (Tp / p - 1) / 3 + 1)
        return hipErrorInvalidValue;
    const int64_t F = (int64_t)B * H0 * p;
    const int S = pd_l0_splits(F);
    const int64_t fs = (F + S - 1) / S;
    hipLaunchKernelGGL(pd_l0_wgrad_kernel, dim3(kPdC0, S), dim3(256), 0, s, dpre, x, scratch, B, T, Tp, H0, p, fs);
    hipLaunchKernelGGL(pd_l0_wgrad_sum_kernel, dim3(1), dim3(256), 0, s, scratch, dw, db, S);
    return hipGetLastError();
}

// gradient of padded sample n of item b: the taps j with 3 ho + j - 2 = n / p, channels in order
__device__ __forceinline__ float pd_l0_dxp(const float* __restrict__ db_, const float* __restrict__ wsm, int n, int H0, int p) {
    const int hi = n / p, wv = n - hi * p, No = H0 * p;
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < kPdTaps; ++j) {
        const int tt = hi + kPdTaps / 2 - j;
        if (tt < 0 || tt % 3 != 0 || tt / 3 >= H0) continue;
        const float* g = db_ + (size_t)(tt / 3) * p + wv;
        for (int co = 0; co < kPdC0; ++co) v = fmaf(wsm[co * kPdTaps + j], g[(size_t)co * No], v);
    }
    return v;
}

// One thread = one sample t < T of one item: its own gradient plus that of the padded sample that mirrors it (n = 2 (T - 1) - t
// in [T, Tp), if any).
__global__ __launch_bounds__(256) void pd_l0_dgrad_kernel(const float* __restrict__ dpre, const float* __restrict__ w, float* __restrict__ dx,
                                                          int T, int Tp, int H0, int p) {
    __shared__ float wsm[kPdC0 * kPdTaps];
    if (threadIdx.x < kPdC0 * kPdTaps) wsm[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const float* db_ = dpre + (size_t)b * kPdC0 * H0 * p;
    float v = pd_l0_dxp(db_, wsm, t, H0, p);
    const int m = 2 * (T - 1) - t;
    if (m >= T && m < Tp) v += pd_l0_dxp(db_, wsm, m, H0, p);
    dx[(size_t)b * T + t] = v;
}

hipError_t launch_pd_l0_dgrad(const float* dpre, const float* w, float* dx, int B, int T, int Tp, int H0, int p, hipStream_t s) {
    if (!dpre || !w || !dx || B < 1 || B > 65535 || T < 1 || p < 1 || Tp < T || Tp % p != 0 || Tp - T >= T || H0 != (Tp / p - 1) / 3 + 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pd_l0_dgrad_kernel, dim3((T + 255) / 256, B), dim3(256), 0, s, dpre, w, dx, T, Tp, H0, p);
    return hipGetLastError();
}

// ---- conv_post -------------------------------------------------------------------------------------------------------------
// One block = 16 frames of one item x 16 channel groups: group g adds channels g, g + 16, ... in order, then thread (g = 0, frame)
// adds the 16 group sums in order.
__global__ __launch_bounds__(256) void pd_post_fwd_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ out, float* __restrict__ out2, int C, int H, int p) {
    __shared__ float red[16][16];
    const int fl = threadIdx.x & 15, g = threadIdx.x >> 4, b = blockIdx.y, No = H * p;
    const int n = blockIdx.x * 16 + fl;
    const bool ok = n < No;
    const int h = ok ? n / p : 0, wv = ok ? n - h * p : 0;
    const float* ib = in + (size_t)b * C * No;
    float v = 0.0f;
    if (ok) {
        for (int ci = g; ci < C; ci += 16) {
#pragma unroll
            for (int j = 0; j < kPdPostTaps; ++j) {
                const int src = h + j - kPdPostTaps / 2;
                if (src >= 0 && src < H) v = fmaf(w[ci * kPdPostTaps + j], ib[((size_t)ci * H + src) * p + wv], v);
            }
        }
    }
    red[g][fl] = v;
    __syncthreads();
    if (g != 0 || !ok) return;
    float sum = red[0][fl];
    for (int k = 1; k < 16; ++k) sum += red[k][fl];
    sum += bias[0];
    out[(size_t)b * No + n] = sum;
    if (out2) out2[(size_t)b * No + n] = sum;
}

hipError_t launch_pd_post_fwd(const float* in, const float* w, const float* bias, float* out, float* out2, int B, int C, int H, int p,
                              hipStream_t s) {
    if (!in || !w || !bias || !out || B < 1 || B > 65535 || C < 1 || H < 1 || p < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pd_post_fwd_kernel, dim3((H * p + 15) / 16, B), dim3(256), 0, s, in, w, bias, out, out2, C, H, p);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void pd_post_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, const float* __restrict__ act,
                                                            const float* __restrict__ addg, float* __restrict__ dpre, int C, int H, int p,
                                                            float slope, int64_t total) {
    const int No = H * p;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t bc = i / No;
        const int n = (int)(i - bc * No), h = n / p, wv = n - h * p;
        const int64_t b = bc / C;
        const int ci = (int)(bc - b * C);
        float v = 0.0f;
        if (dy) {
#pragma unroll
            for (int j = 0; j < kPdPostTaps; ++j) {
                const int ho = h + kPdPostTaps / 2 - j;
                if (ho >= 0 && ho < H) v = fmaf(w[ci * kPdPostTaps + j], dy[(size_t)b * No + (size_t)ho * p + wv], v);
            }
        }
        if (addg) v += addg[i];
        dpre[i] = v * (act[i] > 0.0f ? 1.0f : slope);
    }
}

hipError_t launch_pd_post_dgrad(const float* dy, const float* w, const float* act, const float* addg, float* dpre, int B, int C, int H, int p,
                                float slope, hipStream_t s) {
    if (!w || !act || !dpre || B < 1 || C < 1 || H < 1 || p < 1) return hipErrorInvalidValue;
    const int64_t total = (int64_t)B * C * H * p;
    hipLaunchKernelGGL(pd_post_dgrad_kernel, dim3(grid_1d(total, 4096)), dim3(256), 0, s, dy, w, act, addg, dpre, C, H, p, slope, total);
    return hipGetLastError();
}

// One block per channel: the (item, frame) pairs in strides of 256, a fixed LDS tree
__global__ __launch_bounds__(256) void pd_post_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ in, float* __restrict__ dw,
                                                            int B, int C, int H, int p) {
    __shared__ float red[kPdPostTaps][256];
    const int ci = blockIdx.x, tid = threadIdx.x, No = H * p;
    const int64_t F = (int64_t)B * No;
    float acc[kPdPostTaps];
#pragma unroll
    for (int j = 0; j < kPdPostTaps; ++j) acc[j] = 0.0f;
    for (int64_t f = tid; f < F; f += 256) {
        const int b = (int)(f / No), n = (int)(f - (int64_t)b * No);
        const int h = n / p, wv = n - h * p;
        const float g = dy[f];
        const float* ib = in + ((size_t)b * C + ci) * No;
#pragma unroll
        for (int j = 0; j < kPdPostTaps; ++j) {
            const int src = h + j - kPdPostTaps / 2;
            if (src >= 0 && src < H) acc[j] = fmaf(g, ib[(size_t)src * p + wv], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < kPdPostTaps; ++j) red[j][tid] = acc[j];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int j = 0; j < kPdPostTaps; ++j) red[j][tid] += red[j][tid + w];
        }
        __syncthreads();
    }
    if (tid < kPdPostTaps) dw[ci * kPdPostTaps + tid] = red[tid][0];
}

hipError_t launch_pd_post_wgrad(const float* dy, const float* in, float* dw, int B, int C, int H, int p, hipStream_t s) {
    if (!dy || !in || !dw || B < 1 || C < 1 || H < 1 || p < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pd_post_wgrad_kernel, dim3(C), dim3(256), 0, s, dy, in, dw, B, C, H, p);
    return hipGetLastError();
}

// ---- weight norm -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pd_weight_norm_kernel(const float* __restrict__ v, const float* __restrict__ g, float* __restrict__ w, int n) {
    __shared__ float red[256];
    const int co = blockIdx.x, tid = threadIdx.x;
    const float* vr = v + (size_t)co * n;
    float ss = 0.0f;
    for (int i = tid; i < n; i += 256) ss = fmaf(vr[i], vr[i], ss);
    const float scale = g[co] / sqrtf(block_sum256(red, ss));
    for (int i = tid; i < n; i += 256) w[(size_t)co * n + i] = vr[i] * scale;
}

hipError_t launch_pd_weight_norm(const float* v, const float* g, float* w, int Cout, int n, hipStream_t s) {
    if (!v || !g || !w || Cout < 1 || n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pd_weight_norm_kernel, dim3(Cout), dim3(256), 0, s, v, g, w, n);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void pd_weight_norm_bwd_kernel(const float* __restrict__ dw, const float* __restrict__ v, const float* __restrict__ g,
                                                                 float* __restrict__ dv, float* __restrict__ dg, int n) {
    __shared__ float r1[256], r2[256];
    const int co = blockIdx.x, tid = threadIdx.x;
    const float* vr = v + (size_t)co * n;
    const float* dr = dw + (size_t)co * n;
    float ss = 0.0f, dot = 0.0f;
    for (int i = tid; i < n; i += 256) { ss = fmaf(vr[i], vr[i], ss); dot = fmaf(dr[i], vr[i], dot); }
    r1[tid] = ss; r2[tid] = dot;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) { r1[tid] += r1[tid + k]; r2[tid] += r2[tid + k]; }
        __syncthreads();
    }
    const float inv = 1.0f / sqrtf(r1[0]);
    const float dgv = r2[0] * inv, sc = g[co] * inv;
    if (tid == 0) dg[co] = dgv;
    for (int i = tid; i < n; i += 256) dv[(size_t)co * n + i] = sc * (dr[i] - vr[i] * inv * dgv);
}

hipError_t launch_pd_weight_norm_bwd(const float* dw, const float* v, const float* g, float* dv, float* dg, int Cout, int n, hipStream_t s) {
    if (!dw || !v || !g || !dv || !dg || Cout < 1 || n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pd_weight_norm_bwd_kernel, dim3(Cout), dim3(256), 0, s, dw, v, g, dv, dg, n);
    return hipGetLastError();
}

}  // namespace st
