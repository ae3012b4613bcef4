// Launcher interface of the feature front end (audio_kernels.hip): waveform -> linear / log-mel spectrogram, and its backward.
// Reference: utils/audio.py:19-26 (LinearSpectrogram.forward), :44-52 (MelScale, compress); config.py:4-19.
//
// Backward (vocoders/vocos/models/loss.py differentiates the log-mel of the generator's output).  Per frame t of an utterance,
// f_t[n] = w[n] x[s(t hop + n)], X = rfft(f_t), mag = sqrt(|X|^2 + 1e-6), mel = fb^T mag, y = log(max(mel, 1e-5)); for an
// upstream gradient g of y's shape:
//   1. dmel_m = g_m / mel_m where mel_m >= 1e-5, else 0     (linear spectrogram: dmag = g, steps 1-2 skipped)
//   2. dmag_k = sum_m fb[k, m] dmel_m
//   3. G_k = dmag_k X_k / mag_k
//   4. df_t[n] = Re sum_{k=0}^{N/2} G_k e^{+2 pi i k n / N} = N irfft(C)[n], C_0 = Re G_0, C_{N/2} = Re G_{N/2}, C_k = G_k / 2
//   5. dx[s] = sum over padded positions q with s(q) = s and frames t covering q of w[q - t hop] df_t[q - t hop]
// mel_bwd_kernel<N> does 1-4 and writes w df_t to a (B, frames, N) workspace; mel_gather_kernel does 5.
#pragma once
#include <hip/hip_runtime.h>

namespace st {

constexpr int kMelMinNfft = 32, kMelMaxNfft = 2048;

// One utterance of a ragged launch; entry [B] is a sentinel whose tile0 is the launch's tile count.
struct MelUtt {
    long long s_off;      // first sample in `wave`
    long long f_off;      // output block at out + rows * f_off, (rows, frames)
    int L, frames, tile0, pad_;
};

struct MelArgs {
    const float* wave;
    const float* window;       // (n_fft)
    const float* wband;        // packed nonzero filter weights: filter m's bins lo..hi-1 at wband[off ..]
    const int* band;           // [n_mels][3] = lo, hi, off
    float* out;
    int n_fft, hop, pad;
    int rows;                  // n_mels (log-mel) or n_fft / 2 + 1 (linear magnitude)
    int log_mel;               // 1: project on the bands + log(clamp(., 1e-5)); 0: the magnitude itself
    const MelUtt* utt;         // ragged table (B + 1 entries), or nullptr: B utterances of L samples, frames each
    int B;
    long long L;
    int frames, tiles_per;
    int total_tiles;
};

struct MelBwdArgs {
    const float* wave;         // (B, L)
    const float* window;
    const float* grad;         // (B, rows, frames): the upstream gradient
    const float* wband;        // the forward's filter-major band table (MelArgs)
    const int* band;
    const float* wbandT;       // bin-major: bin k's nonzero weights fb[k, mlo..mhi-1] at wbandT[off ..]
    const int* bandT;          // [n_fft / 2 + 1][3] = mlo, mhi, off
    float* ws;                 // (B, frames, n_fft) workspace: w * df_t
    float* out;                // (B, L) input gradient, overwritten
    int n_fft, hop, pad;
    int rows;                  // n_mels (log-mel, rows <= 2 n_fft) or n_fft / 2 + 1
    int log_mel;
    int B;
    long long L;
    int frames, tiles_per, total_tiles;
};

// frames per block of the n_fft kernel (consecutive frames of one utterance)
int mel_tile_frames(int n_fft);
hipError_t launch_mel(const MelArgs& a, hipStream_t s);
// mel_bwd_kernel<n_fft> over total_tiles blocks, then the gather kernel over B * L samples, on one stream
hipError_t launch_mel_backward(const MelBwdArgs& a, hipStream_t s);
// step 5 alone: the gather of a (B, frames, n_fft) workspace of windowed frame gradients onto the samples (reads ws, n_fft, hop, pad,
// B, L, frames; writes out), for a caller that fills the workspace itself (resolution_disc_kernels.hip)
hipError_t launch_mel_gather(const MelBwdArgs& a, hipStream_t s);

}  // namespace st
