// Feature front end (utils/audio.py:19-26,44-52): waveform -> |STFT| -> mel bands -> log, all fp32.
//
// One block (256 threads) = FR consecutive frames of one utterance.  A frame of n_fft = N samples is read straight from the
// waveform with torch's reflect padding as index arithmetic (padded position q -> sample s = q - pad; s < 0 reads -s,
// s >= L reads 2 (L - 1) - s), multiplied by the window and transformed as ONE complex FFT of H = N / 2 points,
//     z[n] = x[2n] + i x[2n+1],   Z = FFT_H(z),
//     X[k] = (Z[k] + conj Z[H-k]) / 2 - (i / 2) e^{-2 pi i k / N} (Z[k] - conj Z[H-k])      (k = 0..H, indices mod H)
// -- the mirror image of the ISTFT pre-pass in vocos_kernels.hip.  The H-point transform is radix-4 Stockham autosort
// passes between two LDS buffers (plus one radix-2 pass when log2 H is odd) over S = 1024 / H frames at a time, so that
// every pass has one butterfly per thread.  The magnitudes of the tile's FR frames stay in LDS; the mel projection then
// sums each filter's nonzero bins only (band table of st_finalize), in ascending bin order, and writes each mel row's
// run of frames contiguously in the channel-major output.
#include "audio_launch.h"

namespace st {
namespace {

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

template <int N>
__global__ __launch_bounds__(256) void mel_kernel(MelArgs a) {
    using G = MelGeo<N>;
    constexpr int H = G::H, S = G::S, FR = G::FR, Q = G::Q;
    __shared__ float2 buf[2][S * H];                // 16 KiB for every N
    __shared__ float2 tw[H];                        // e^{-2 pi i m / N}, m < H
    __shared__ float mag[FR * (H + 1)];             // the tile's magnitudes, [frame][bin]
    const int tid = threadIdx.x;
    const int blk = blockIdx.x;

    // which utterance and tile: the ragged table (uniform binary search), or B equal utterances
    long long s_off, f_off, L;
    int frames, tile;
    if (a.utt) {
        int lo = 0, hi = a.B;                       // utt[lo].tile0 <= blk < utt[hi].tile0
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.utt[mid].tile0 <= blk) lo = mid; else hi = mid;
        }
        const MelUtt u = a.utt[lo];
        s_off = u.s_off; f_off = u.f_off; L = u.L; frames = u.frames; tile = blk - u.tile0;
    } else {
        const int b = blk / a.tiles_per;
        tile = blk - b * a.tiles_per;
        L = a.L; frames = a.frames; s_off = (long long)b * a.L; f_off = (long long)b * a.frames;
    }
    const int t0 = tile * FR;
    const float* __restrict__ x = a.wave + s_off;
    const float* __restrict__ win = a.window;

    for (int m = tid; m < H; m += 256) {
        float sn, cs;
        sincospif((float)(2 * m) / (float)N, &sn, &cs);
        tw[m] = make_float2(cs, -sn);
    }

#pragma unroll 1
    for (int r = 0; r < FR / S; ++r) {
        // framing + window: buf[0] viewed as [S][N] floats is z = x[2n] + i x[2n+1] of each frame
        float* z = reinterpret_cast<float*>(buf[0]);
        for (int e = tid; e < S * N; e += 256) {
            const int f = e / N, m = e & (N - 1);
            const int t = t0 + r * S + f;
            float v = 0.0f;
            if (t < frames) {
                long long q = (long long)t * a.hop + m - a.pad;
                if (q < 0) q = -q;
                if (q >= L) q = 2 * (L - 1) - q;
                v = x[q] * win[m];
            }
            z[e] = v;
        }
        __syncthreads();

        float2* in = buf[0];
        float2* out = buf[1];
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

        // split pass to the N-point real spectrum and its magnitude (utils/audio.py:24-25)
        for (int e = tid; e < S * (H + 1); e += 256) {
            const int f = e / (H + 1), k = e - f * (H + 1);
            const float2 A = in[f * H + (k & (H - 1))], Bz = in[f * H + ((H - k) & (H - 1))];
            const float2 E = make_float2(0.5f * (A.x + Bz.x), 0.5f * (A.y - Bz.y));
            const float2 O = make_float2(0.5f * (A.x - Bz.x), 0.5f * (A.y + Bz.y));
            const float2 P = cmulf(twn(tw, k, H), O);
            const float re = E.x + P.y, im = E.y - P.x;
            mag[(r * S + f) * (H + 1) + k] = sqrtf(re * re + im * im + 1e-6f);
        }
        __syncthreads();
    }

    const int nvalid = frames - t0 < FR ? frames - t0 : FR;
    float* __restrict__ o = a.out + (f_off * a.rows + t0);       // row c of this utterance at o + c * frames
    if (!a.log_mel) {
        for (int e = tid; e < (H + 1) * FR; e += 256) {
            const int k = e / FR, f = e & (FR - 1);
            if (f < nvalid) o[(long long)k * frames + f] = mag[f * (H + 1) + k];
        }
        return;
    }
    for (int e = tid; e < a.rows * FR; e += 256) {                // mel_scale (:44-45) + compress (:47-48)
        const int m = e / FR, f = e & (FR - 1);
        if (f >= nvalid) continue;
        const int lo = a.band[3 * m], hi = a.band[3 * m + 1];
        const float* __restrict__ w = a.wband + a.band[3 * m + 2] - lo;
        const float* __restrict__ mg = mag + f * (H + 1);
        float acc = 0.0f;
        for (int k = lo; k < hi; ++k) acc += w[k] * mg[k];
        o[(long long)m * frames + f] = logf(acc < 1e-5f ? 1e-5f : acc);      // NaN passes like torch.clamp
    }
}

template <int N>
hipError_t launch_n(const MelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((mel_kernel<N>), dim3((unsigned)a.total_tiles), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace

int mel_tile_frames(int n_fft) {
    const int S = 2048 / n_fft;
    return S > 8 ? S : 8;
}

hipError_t launch_mel(const MelArgs& a, hipStream_t s) {
    if (a.total_tiles <= 0) return hipSuccess;
    switch (a.n_fft) {
        case 32: return launch_n<32>(a, s);
        case 64: return launch_n<64>(a, s);
        case 128: return launch_n<128>(a, s);
        case 256: return launch_n<256>(a, s);
        case 512: return launch_n<512>(a, s);
        case 1024: return launch_n<1024>(a, s);
        case 2048: return launch_n<2048>(a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace st
