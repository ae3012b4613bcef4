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
//
// Backward (audio_launch.h, steps 1-5): mel_bwd_kernel<N> reuses the framing, FFT and split device functions, so the spectrum and
// the mel sums it differentiates are bitwise the forward's; mel_gather_kernel sums each sample's frame terms without atomics.
// The framing, FFT, split and inverse device functions live in audio_fft.h, which resolution_disc_kernels.hip shares.
#include "audio_fft.h"
#include "audio_launch.h"

namespace st {
namespace {

template <int N>
__global__ __launch_bounds__(256) void mel_kernel(MelArgs a) {
    using G = MelGeo<N>;
    constexpr int H = G::H, S = G::S, FR = G::FR;
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

    mel_twiddles<N>(tw, tid);

#pragma unroll 1
    for (int r = 0; r < FR / S; ++r) {
        // framing + window: buf[0] viewed as [S][N] floats is z = x[2n] + i x[2n+1] of each frame
        mel_frame_load<N>(reinterpret_cast<float*>(buf[0]), x, win, t0 + r * S, frames, a.hop, a.pad, L, tid);
        __syncthreads();
        const float2* in = mel_fft<N>(buf[0], buf[1], tw, tid);

        // split pass to the N-point real spectrum and its magnitude (utils/audio.py:24-25)
        for (int e = tid; e < S * (H + 1); e += 256) {
            const int f = e / (H + 1), k = e - f * (H + 1);
            const float2 X = mel_split_bin<N>(in, tw, f, k);
            mag[(r * S + f) * (H + 1) + k] = sqrtf(X.x * X.x + X.y * X.y + 1e-6f);
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

// Backward, steps 1-4 of the header comment in audio_launch.h: per frame, the spectrum X and (log-mel) mel_m recomputed exactly as
// mel_kernel computes them, then dmel = g / mel (0 under the clamp), dmag = fb dmel (bin-major band table), G = dmag X / mag,
// C = the half-spectrum of the inverse real FFT, and w * (N irfft(C)) written to the frame's row of the workspace.  The inverse
// is the mirror of the split pass: Z'_k = (C_k + conj C_{H-k}) + i e^{+2 pi i k / N} (C_k - conj C_{H-k}), k < H, and
// IFFT_H(Z') = conj FFT_H(conj Z') holds N df[2n] + i N df[2n+1].  Same tiling and grid as the forward, S frames per round.
template <int N>
__global__ __launch_bounds__(256) void mel_bwd_kernel(MelBwdArgs a) {
    using G = MelGeo<N>;
    constexpr int H = G::H, S = G::S, FR = G::FR;
    __shared__ float2 buf[2][S * H];                // FFT ping-pong; between the passes [S][rows] floats of dmel (rows <= 2 N)
    __shared__ float2 tw[H];
    __shared__ float2 spec[S * (H + 1)];            // X of the round's frames, then C
    __shared__ float mag[S * (H + 1)];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.tiles_per;
    const int t0 = (blockIdx.x - b * a.tiles_per) * FR;
    const int frames = a.frames, rows = a.rows;
    const float* __restrict__ x = a.wave + (long long)b * a.L;
    const float* __restrict__ win = a.window;
    const float* __restrict__ g = a.grad + (long long)b * rows * frames;       // (rows, frames) of this utterance
    float* __restrict__ ws = a.ws + (long long)b * frames * N;                 // (frames, N)

    mel_twiddles<N>(tw, tid);

#pragma unroll 1
    for (int r = 0; r < FR / S; ++r) {
        const int tr = t0 + r * S;
        if (tr >= frames) break;                                              // block-uniform
        mel_frame_load<N>(reinterpret_cast<float*>(buf[0]), x, win, tr, frames, a.hop, a.pad, a.L, tid);
        __syncthreads();
        const float2* Z = mel_fft<N>(buf[0], buf[1], tw, tid);
        for (int e = tid; e < S * (H + 1); e += 256) {
            const int f = e / (H + 1), k = e - f * (H + 1);
            const float2 X = mel_split_bin<N>(Z, tw, f, k);
            spec[e] = X;
            mag[e] = sqrtf(X.x * X.x + X.y * X.y + 1e-6f);
        }
        __syncthreads();

        // 1. dmel_m = g_m / mel_m where mel_m >= 1e-5 (torch.clamp's mask), else 0; mel_m summed as mel_kernel sums it
        float* dmel = reinterpret_cast<float*>(&buf[0][0]);
        if (a.log_mel) {
            for (int e = tid; e < S * rows; e += 256) {
                const int f = e / rows, m = e - f * rows;
                const int t = tr + f;
                float d = 0.0f;
                if (t < frames) {
                    const int lo = a.band[3 * m], hi = a.band[3 * m + 1];
                    const float* __restrict__ w = a.wband + a.band[3 * m + 2] - lo;
                    const float* __restrict__ mg = mag + f * (H + 1);
                    float acc = 0.0f;
                    for (int k = lo; k < hi; ++k) acc += w[k] * mg[k];
                    d = acc >= 1e-5f ? g[(long long)m * frames + t] / acc : 0.0f;
                }
                dmel[e] = d;
            }
            __syncthreads();
        }

        // 2-3. dmag_k = sum_m fb[k, m] dmel_m (ascending m), G_k = dmag_k X_k / mag_k, and C_k (halved off the two real bins)
        for (int e = tid; e < S * (H + 1); e += 256) {
            const int f = e / (H + 1), k = e - f * (H + 1);
            const int t = tr + f;
            float dmag = 0.0f;
            if (t < frames) {
                if (a.log_mel) {
                    const int lo = a.bandT[3 * k], hi = a.bandT[3 * k + 1];
                    const float* __restrict__ w = a.wbandT + a.bandT[3 * k + 2] - lo;
                    const float* __restrict__ dm = dmel + f * rows;
                    for (int m = lo; m < hi; ++m) dmag += w[m] * dm[m];
                } else {
                    dmag = g[(long long)k * frames + t];
                }
            }
            const float sc = dmag / mag[e];
            const float2 X = spec[e];
            spec[e] = (k == 0 || k == H) ? make_float2(sc * X.x, 0.0f) : make_float2(0.5f * (sc * X.x), 0.5f * (sc * X.y));
        }
        __syncthreads();

        // 4. the inverse real FFT of C, windowed, into the frame's row of the workspace
        mel_inverse_to_ws<N>(spec, buf[0], buf[1], tw, ws, win, tr, frames, tid);
        __syncthreads();                                                       // buf is the next round's frame buffer
    }
}

// 5. dx[s] = sum over the padded positions q that read s (direct q = s + pad; left reflection q = pad - s for 1 <= s <= pad; right
// reflection q = 2 (L - 1) - s + pad for s <= L - 2) and the frames t whose window covers q, of ws[t][q - t hop]: in that order of
// positions and ascending t, one thread per sample, no atomics.
__global__ __launch_bounds__(256) void mel_gather_kernel(MelBwdArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.B * a.L) return;
    const long long b = i / a.L, s = i - b * a.L, L = a.L;
    const int N = a.n_fft, hop = a.hop, frames = a.frames;
    const float* __restrict__ ws = a.ws + b * frames * N;
    float acc = 0.0f;
    auto add = [&](long long q) {
        const long long tlo = q < N ? 0 : (q - N + hop) / hop;                // first t with q < t hop + N
        long long thi = q / hop;
        if (thi > frames - 1) thi = frames - 1;
        for (long long t = tlo; t <= thi; ++t) acc += ws[t * N + (q - t * hop)];
    };
    add(s + a.pad);
    if (s >= 1 && s <= a.pad) add(a.pad - s);
    if (s <= L - 2) add(2 * (L - 1) - s + a.pad);
    a.out[i] = acc;
}

template <int N>
hipError_t launch_n(const MelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((mel_kernel<N>), dim3((unsigned)a.total_tiles), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int N>
hipError_t launch_bwd_n(const MelBwdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((mel_bwd_kernel<N>), dim3((unsigned)a.total_tiles), dim3(256), 0, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const long long n = (long long)a.B * a.L;
    hipLaunchKernelGGL(mel_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
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

hipError_t launch_mel_gather(const MelBwdArgs& a, hipStream_t s) {
    const long long n = (long long)a.B * a.L;
    if (n <= 0 || !a.ws || !a.out || a.frames < 1 || a.hop < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mel_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mel_backward(const MelBwdArgs& a, hipStream_t s) {
    if (a.total_tiles <= 0) return hipSuccess;
    switch (a.n_fft) {
        case 32: return launch_bwd_n<32>(a, s);
        case 64: return launch_bwd_n<64>(a, s);
        case 128: return launch_bwd_n<128>(a, s);
        case 256: return launch_bwd_n<256>(a, s);
        case 512: return launch_bwd_n<512>(a, s);
        case 1024: return launch_bwd_n<1024>(a, s);
        case 2048: return launch_bwd_n<2048>(a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace st
