// Monotonic alignment search of StableTTS training (models/model.py:148-158): the fused neg_cent and the maximum_path
// dynamic program with its backtrack (monotonic_align/core.py:14-46), on the device instead of a host round trip.
// The DP is fp32 adds and compares with an integer result, so it is reproduced bit for bit: no fast-math, no contraction
// (build.py EXTRA_FLAGS), Python's max as the select `v_cur > v_prev ? v_cur : v_prev`.
#include "mas_launch.h"

#include <math.h>

namespace st {

typedef __attribute__((ext_vector_type(16))) float mas_f32x16;

constexpr float kMasNeg = -1e9f;          // max_neg_val (core.py:21), exact in fp32
constexpr int kDppWaveShr1 = 0x138;       // DPP wave_shr:1: lane l reads lane l - 1 of the whole wave; lane 0 keeps `old`

// x - 1 neighbour of a wave-strided row: lane l gets v from lane l - 1, lane 0 gets lane0 (column 64k - 1, from group k - 1)
__device__ __forceinline__ float mas_shift_up1(float v, float lane0) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0), __float_as_int(v), kDppWaveShr1, 0xf, 0xf, false));
}

// v with lane j replaced by the uniform value u
__device__ __forceinline__ int mas_setlane(int v, int j, int u) { return (int)threadIdx.x == j ? u : v; }

__device__ __forceinline__ unsigned long long mas_readlane64(unsigned lo, unsigned hi, int j) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, j) << 32) | (unsigned)__builtin_amdgcn_readlane((int)lo, j);
}

struct MasPathArgs {
    const float* neg_cent; const int32_t* t_y; const int32_t* t_x;
    float* path; int32_t* durations; unsigned long long* ws;
    int Ty, Tx;
};

// One wave = one utterance.  Row y of the value table lives in registers, column x = 64 k + lane in st[k] (K >= ceil(Tx/64)
// groups); raw neg_cent rows are prefetched P rows ahead into a register ring (their loads do not depend on the DP chain).
// Per row, every column x < t_x emits the backtrack's decision bit value[y-1, x] < value[y-1, x-1] on the accumulated-or-raw
// row (one __ballot per group gives the row's 64-bit words) -- over every column, not only the band, which is what makes
// t_x > t_y exact.  Words go to LDS (LDS = true) or to the global workspace.  The backtrack then walks 64 rows per window: lane j
// fetches the two words of row ytop - j - 1 around the current index (the index drops by at most one per row), the walk
// itself is scalar, and each output row is written whole (zeros and the one 1).
template <int K, int P, bool LDS>
__global__ __launch_bounds__(64) void mas_path_kernel(MasPathArgs a) {
    extern __shared__ unsigned long long mas_lds_bits[];
    const int lane = threadIdx.x, b = blockIdx.x;
    const int Ty = a.Ty, Tx = a.Tx, Kn = (Tx + 63) >> 6;
    const int ty = min(max(a.t_y[b], 0), Ty), tx = min(max(a.t_x[b], 0), Tx);
    const float* src = a.neg_cent + (size_t)b * Ty * Tx;
    float* dst = a.path + (size_t)b * Ty * Tx;
    unsigned long long* bits = LDS ? mas_lds_bits : a.ws + (size_t)b * Ty * Kn;
    int32_t* dur = a.durations ? a.durations + (size_t)b * Tx : nullptr;
    int y_end = 0;                        // rows [y_end, Ty) are zero rows
    if (ty > 0 && tx > 0) {
        float st[K], ring[P][K];
        // clamped addresses: every load is in bounds and unconditional; columns >= t_x and rows >= t_y are never used
        auto load_row = [&](float (&r)[K], int row) {
            const float* rp = src + (size_t)min(row, ty - 1) * Tx;
#pragma unroll
            for (int k = 0; k < K; ++k) r[k] = rp[min(k * 64 + lane, tx - 1)];
        };
#pragma unroll
        for (int p = 0; p < P; ++p) load_row(ring[p], p);
#pragma unroll
        for (int k = 0; k < K; ++k) st[k] = 0.0f;
        for (int y0 = 0; y0 < ty; y0 += P) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int y = y0 + p;
                if (y >= ty) break;
                const int lo = max(0, tx + y - ty), hi = min(tx, y + 1);
                int wlo = 0, whi = 0;     // decision word of row y - 1, group `lane` (lanes < Kn)
                float carry = 0.0f;       // column 64 k - 1 of row y - 1
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int x = k * 64 + lane;
                    const float old = st[k];                     // value[y - 1, x], accumulated or raw
                    const float nb = mas_shift_up1(old, carry);  // value[y - 1, x - 1]
                    carry = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(old), 63));
                    const unsigned long long w = __ballot(x >= 1 && x < tx && old < nb);     // (row -1 at y = 0: not stored)
                    wlo = mas_setlane(wlo, k, (int)(unsigned)w);
                    whi = mas_setlane(whi, k, (int)(unsigned)(w >> 32));
                    const float v_cur = x == y ? kMasNeg : old;
                    const float v_prev = x == 0 ? (y == 0 ? 0.0f : kMasNeg) : nb;
                    const float m = v_cur > v_prev ? v_cur : v_prev;
                    const float raw = ring[p][k];
                    st[k] = (x >= lo && x < hi) ? raw + m : raw;
                }
                if (y > 0 && lane < Kn) bits[(size_t)(y - 1) * Kn + lane] = ((unsigned long long)(unsigned)whi << 32) | (unsigned)wlo;
                load_row(ring[p], y + P);
            }
        }
        __syncthreads();                  // the walk reads words other lanes wrote

        int idx = tx - 1, cnt = 0;
        for (int ytop = ty - 1; ytop >= 0; ytop -= 64) {
            const int n = min(64, ytop + 1), g0 = idx >> 6;
            const int r = ytop - lane;                       // this lane's row of the window
            unsigned long long w1 = 0, w0 = 0;                 // words of row r - 1: groups g0 and g0 - 1
            if (lane < n && r >= 1) {
                w1 = bits[(size_t)(r - 1) * Kn + g0];
                if (g0 >= 1) w0 = bits[(size_t)(r - 1) * Kn + g0 - 1];
            }
            const unsigned w1l = (unsigned)w1, w1h = (unsigned)(w1 >> 32), w0l = (unsigned)w0, w0h = (unsigned)(w0 >> 32);
            int pidx = 0, left = -1, lcnt = 0;   // lane j: path column of row ytop - j; token left below that row, its frames
            for (int j = 0; j < n; ++j) {
                const int y = ytop - j;
                pidx = mas_setlane(pidx, j, idx);
                ++cnt;
                if (y >= 1 && idx != 0) {
                    bool mv = idx == y;
                    if (!mv) {
                        const unsigned long long w = (idx >> 6) == g0 ? mas_readlane64(w1l, w1h, j) : mas_readlane64(w0l, w0h, j);
                        mv = (w >> (idx & 63)) & 1ull;
                    }
                    if (mv) {
                        left = mas_setlane(left, j, idx);
                        lcnt = mas_setlane(lcnt, j, cnt);
                        --idx;
                        cnt = 0;
                    }
                }
            }
            if (dur && left >= 0) dur[left] = lcnt;
            for (int j = 0; j < n; ++j) {
                const int col = __builtin_amdgcn_readlane(pidx, j);
                float* rowp = dst + (size_t)(ytop - j) * Tx;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int x = k * 64 + lane;
                    if (x < Tx) rowp[x] = x == col ? 1.0f : 0.0f;
                }
            }
        }
        if (dur)
            for (int x = lane; x < Tx; x += 64)
                if (x <= idx || x >= tx) dur[x] = x == idx ? cnt : 0;
        y_end = ty;
    } else if (dur) {
        for (int x = lane; x < Tx; x += 64) dur[x] = 0;
    }
    for (int row = y_end; row < Ty; ++row) {
        float* rowp = dst + (size_t)row * Tx;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int x = k * 64 + lane;
            if (x < Tx) rowp[x] = 0.0f;
        }
    }
}

static size_t mas_bits_bytes(int Ty, int Tx) { return (size_t)Ty * (size_t)((Tx + 63) / 64) * 8; }

size_t mas_workspace_bytes(int B, int Ty, int Tx) {
    if (B < 1 || Ty < 1 || Tx < 1) return 0;
    const size_t per = mas_bits_bytes(Ty, Tx);
    return per <= kMasLdsBudget ? 0 : (size_t)B * per;
}

template <int K, int P>
static hipError_t launch_mas_path_k(const MasPathArgs& a, int B, hipStream_t s) {
    const size_t per = mas_bits_bytes(a.Ty, a.Tx);
    if (per <= kMasLdsBudget) hipLaunchKernelGGL((mas_path_kernel<K, P, true>), dim3(B), dim3(64), per, s, a);
    else hipLaunchKernelGGL((mas_path_kernel<K, P, false>), dim3(B), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mas_path(const float* neg_cent, const int32_t* t_y, const int32_t* t_x, int B, int Ty, int Tx, float* path,
                           int32_t* durations, void* workspace, hipStream_t s) {
    if (B < 1 || Ty < 1 || Tx < 1 || Tx > kMasMaxTx || !neg_cent || !t_y || !t_x || !path) return hipErrorInvalidValue;
    if (mas_workspace_bytes(B, Ty, Tx) && !workspace) return hipErrorInvalidValue;
    const MasPathArgs a{neg_cent, t_y, t_x, path, durations, (unsigned long long*)workspace, Ty, Tx};
    const int kn = (Tx + 63) / 64;
    // register plan: K groups of state + a P-row prefetch ring (P K <= 64 from K = 8 up, at least 2 rows)
    if (kn <= 1) return launch_mas_path_k<1, 16>(a, B, s);
    if (kn <= 2) return launch_mas_path_k<2, 16>(a, B, s);
    if (kn <= 4) return launch_mas_path_k<4, 16>(a, B, s);
    if (kn <= 8) return launch_mas_path_k<8, 8>(a, B, s);
    if (kn <= 16) return launch_mas_path_k<16, 4>(a, B, s);
    if (kn <= 32) return launch_mas_path_k<32, 2>(a, B, s);
    return launch_mas_path_k<64, 2>(a, B, s);
}

// ---- neg_cent (models/model.py:150-155, s_p_sq_r = 1): a batched TN GEMM on the fp32-input MFMA with a norm epilogue.
// One block = 4 waves = a 64 (frames t) x 64 (tokens s) tile; wave w owns the 32 x 32 sub-tile (t: 32 (w & 1), s: 32 (w >> 1)).
// MFMA 32x32x2 f32 operands: lane l holds A[i = l & 31][k = l >> 5] = y[d][t] and B[k = l >> 5][j = l & 31] = mu_x[d][s];
// D: row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31.  The two column norms are summed from the same LDS chunks, once
// per column of the tile (waves 0 and 1), in d order.
constexpr int kNcTile = 64, kNcChunk = 16;

__global__ __launch_bounds__(256) void mas_neg_cent_kernel(const float* __restrict__ mu_x, const float* __restrict__ y, int D,
                                                           int Tx, int Ty, float c1, float* __restrict__ out) {
    __shared__ float Ys[kNcChunk][kNcTile];
    __shared__ float Ms[kNcChunk][kNcTile];
    __shared__ float ny[kNcTile], nm[kNcTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5, wt = wave & 1, ws = wave >> 1;
    const int s0 = blockIdx.x * kNcTile, t0 = blockIdx.y * kNcTile, b = blockIdx.z;
    const float* yb = y + (size_t)b * D * Ty;
    const float* mb = mu_x + (size_t)b * D * Tx;
    mas_f32x16 acc;
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    float nacc = 0.0f;        // wave 0: sum_d y^2 of frame t0 + lane; wave 1: sum_d mu_x^2 of token s0 + lane
    for (int d0 = 0; d0 < D; d0 += kNcChunk) {
        for (int i = tid; i < kNcChunk * kNcTile; i += 256) {
            const int dd = i / kNcTile, c = i - dd * kNcTile, d = d0 + dd;
            Ys[dd][c] = (d < D && t0 + c < Ty) ? yb[(size_t)d * Ty + t0 + c] : 0.0f;
            Ms[dd][c] = (d < D && s0 + c < Tx) ? mb[(size_t)d * Tx + s0 + c] : 0.0f;
        }
        __syncthreads();
        if (wave < 2) {
            const float* col = wave == 0 ? &Ys[0][lane] : &Ms[0][lane];
            for (int dd = 0; dd < kNcChunk; ++dd) nacc = fmaf(col[dd * kNcTile], col[dd * kNcTile], nacc);
        }
#pragma unroll
        for (int kk = 0; kk < kNcChunk; kk += 2) {
            const float av = Ys[kk + h][wt * 32 + r];
            const float bv = Ms[kk + h][ws * 32 + r];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    if (wave == 0) ny[lane] = -0.5f * nacc;
    else if (wave == 1) nm[lane] = -0.5f * nacc;
    __syncthreads();
    const int sl = ws * 32 + r, s = s0 + sl;
    if (s >= Tx) return;
    const float n4 = nm[sl];
    float* ob = out + (size_t)b * Ty * Tx;
    for (int i = 0; i < 16; ++i) {
        const int tl = wt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h, t = t0 + tl;
        if (t < Ty) ob[(size_t)t * Tx + s] = ((c1 + ny[tl]) + acc[i]) + n4;      // (neg_cent1 + neg_cent2) + neg_cent3 + neg_cent4
    }
}

hipError_t launch_mas_neg_cent(const float* mu_x, const float* y, int B, int D, int Tx, int Ty, float* neg_cent, hipStream_t s) {
    if (B < 1 || B > 65535 || D < 1 || Tx < 1 || Ty < 1 || (Ty + kNcTile - 1) / kNcTile > 65535 || !mu_x || !y || !neg_cent)
        return hipErrorInvalidValue;
    const float c1 = (float)((double)D * (-0.5 * log(2.0 * M_PI)));
    const dim3 grid((Tx + kNcTile - 1) / kNcTile, (Ty + kNcTile - 1) / kNcTile, B);
    hipLaunchKernelGGL(mas_neg_cent_kernel, grid, dim3(256), 0, s, mu_x, y, D, Tx, Ty, c1, neg_cent);
    return hipGetLastError();
}

}  // namespace st
