// The real FFT of the feature front end as device functions, shared by audio_kernels.hip (magnitude / log-mel spectrogram and its
// backward) and resolution_disc_kernels.hip (the complex STFT of the multi-resolution discriminator and its backward): twiddles,
// reflect framing, the H = N / 2 point radix-4 Stockham transform between two LDS buffers, the split pass to the N-point real
// spectrum, and its mirror, the inverse real FFT of a half spectrum.  All for blocks of 256 threads; see audio_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace st {

__device__ __forceinline__ float2 cmulf(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

template <int N>
struct MelGeo {
    static constexpr int H = N / 2;                 // complex FFT length
    static constexpr int S = 1024 / H;              // frames transformed at once (H / 4 radix-4 butterflies each)
    static constexpr int FR = S > 8 ? S : 8;        // frames per block
    static constexpr int Q = H / 4;
};

// e^{-2 pi i m / N} for m in [0, N) from the table of its first half
__device__ __forceinline__ float2 twn(const float2* tw, int m, int H) {
    const float2 w = tw[m < H ? m : m - H];
    return m < H ? w : make_float2(-w.x, -w.y);
}

// ---- the pieces both directions share: twiddles, framing, the H-point FFT, the split pass ----

template <int N>
__device__ __forceinline__ void mel_twiddles(float2* tw, int tid) {
    for (int m = tid; m < N / 2; m += 256) {
        float sn, cs;
        sincospif((float)(2 * m) / (float)N, &sn, &cs);
        tw[m] = make_float2(cs, -sn);
    }
}

// frames t0 .. t0 + S - 1 (zeros past `frames`) windowed into z, viewed as [S][N] floats = z[n] = x[2n] + i x[2n+1] per frame
template <int N>
__device__ __forceinline__ void mel_frame_load(float* z, const float* __restrict__ x, const float* __restrict__ win, int t0,
                                               int frames, int hop, int pad, long long L, int tid) {
    constexpr int S = MelGeo<N>::S;
    for (int e = tid; e < S * N; e += 256) {
        const int f = e / N, m = e & (N - 1);
        const int t = t0 + f;
        float v = 0.0f;
        if (t < frames) {
            long long q = (long long)t * hop + m - pad;
            if (q < 0) q = -q;
            if (q >= L) q = 2 * (L - 1) - q;
            v = x[q] * win[m];
        }
        z[e] = v;
    }
}

// S forward H-point FFTs (e^{-2 pi i ...}) from b0, ping-ponging with b1; returns the buffer that holds the result
template <int N>
__device__ __forceinline__ float2* mel_fft(float2* b0, float2* b1, const float2* tw, int tid) {
    using G = MelGeo<N>;
    constexpr int H = G::H, S = G::S, Q = G::Q;
    float2* in = b0;
    float2* out = b1;
#pragma unroll
    for (int Ns = 1; Ns * 4 <= H; Ns *= 4) {        // radix-4 Stockham passes, one butterfly per thread
        const int f = tid / Q, j = tid - f * Q;
        const int k = j & (Ns - 1);
        const int ts = k * (H / (4 * Ns));          // twiddle e^{-2 pi i r k / (4 Ns)} = W_N^{2 r ts}
        const float2* src = in + f * H;
        const float2 u0 = src[j];
        const float2 u1 = cmulf(src[j + Q], twn(tw, 2 * ts, H));
        const float2 u2 = cmulf(src[j + 2 * Q], twn(tw, 4 * ts, H));
        const float2 u3 = cmulf(src[j + 3 * Q], twn(tw, 6 * ts, H));
        const float2 s02 = make_float2(u0.x + u2.x, u0.y + u2.y), d02 = make_float2(u0.x - u2.x, u0.y - u2.y);
        const float2 s13 = make_float2(u1.x + u3.x, u1.y + u3.y), d13 = make_float2(u1.x - u3.x, u1.y - u3.y);
        float2* dst = out + f * H + ((j - k) << 2) + k;
        dst[0] = make_float2(s02.x + s13.x, s02.y + s13.y);
        dst[Ns] = make_float2(d02.x + d13.y, d02.y - d13.x);          // u0 - i u1 - u2 + i u3
        dst[2 * Ns] = make_float2(s02.x - s13.x, s02.y - s13.y);
        dst[3 * Ns] = make_float2(d02.x - d13.y, d02.y + d13.x);      // u0 + i u1 - u2 - i u3
        __syncthreads();
        float2* tmp = in; in = out; out = tmp;
    }
    if constexpr ((H & 0x55555555) == 0) {           // log2 H odd: one radix-2 pass, Ns = H / 2
        for (int e = tid; e < S * (H / 2); e += 256) {
            const int f = e / (H / 2), j = e - f * (H / 2);
            const float2 v0 = in[f * H + j], v1 = cmulf(in[f * H + j + H / 2], twn(tw, 2 * j, H));
            out[f * H + j] = make_float2(v0.x + v1.x, v0.y + v1.y);
            out[f * H + j + H / 2] = make_float2(v0.x - v1.x, v0.y - v1.y);
        }
        __syncthreads();
        float2* tmp = in; in = out; out = tmp;
    }
    return in;
}

// bin k (0..H) of frame f's N-point real spectrum X from the H-point transform Z of its even / odd samples
template <int N>
__device__ __forceinline__ float2 mel_split_bin(const float2* Z, const float2* tw, int f, int k) {
    constexpr int H = N / 2;
    const float2 A = Z[f * H + (k & (H - 1))], Bz = Z[f * H + ((H - k) & (H - 1))];
    const float2 E = make_float2(0.5f * (A.x + Bz.x), 0.5f * (A.y - Bz.y));
    const float2 O = make_float2(0.5f * (A.x - Bz.x), 0.5f * (A.y + Bz.y));
    const float2 P = cmulf(twn(tw, k, H), O);
    return make_float2(E.x + P.y, E.y - P.x);
}

// Inverse of the split pass for the S frames tr .. tr + S - 1: C (spec, [S][H + 1], C_0 and C_H real, C_k = G_k / 2 between) ->
// conj Z'_k into b0, Z'_k = (C_k + conj C_{H-k}) + i e^{+2 pi i k / N} (C_k - conj C_{H-k}); the forward FFT of it, conjugated, holds
// N df[2n] + i N df[2n+1]; w[n] N df[n] goes to row t of ws (frames, N).  The caller synchronises before it reuses b0 / b1.
template <int N>
__device__ __forceinline__ void mel_inverse_to_ws(const float2* spec, float2* b0, float2* b1, const float2* tw, float* __restrict__ ws,
                                                  const float* __restrict__ win, int tr, int frames, int tid) {
    constexpr int H = MelGeo<N>::H, S = MelGeo<N>::S;
    for (int e = tid; e < S * H; e += 256) {
        const int f = e / H, k = e - f * H;
        const float2 A = spec[f * (H + 1) + k], Bc0 = spec[f * (H + 1) + H - k];
        const float2 Ev = make_float2(A.x + Bc0.x, A.y - Bc0.y);             // C_k + conj C_{H-k}
        const float2 D = make_float2(A.x - Bc0.x, A.y + Bc0.y);              // C_k - conj C_{H-k}
        const float2 w = twn(tw, k, H);
        const float2 P = cmulf(make_float2(w.x, -w.y), D);                   // e^{+2 pi i k / N} D
        b0[e] = make_float2(Ev.x - P.y, -(Ev.y + P.x));                      // conj(Ev + i P)
    }
    __syncthreads();
    const float2* zz = mel_fft<N>(b0, b1, tw, tid);
    for (int e = tid; e < S * N; e += 256) {
        const int f = e / N, n = e & (N - 1);
        const int t = tr + f;
        if (t < frames) {
            const float2 v = zz[f * H + (n >> 1)];
            ws[(long long)t * N + n] = win[n] * ((n & 1) ? -v.y : v.x);
        }
    }
}

}  // namespace st
