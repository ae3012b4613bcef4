// Launcher interface of the feature front end (audio_kernels.hip): waveform -> linear / log-mel spectrogram.
// Reference: utils/audio.py:19-26 (LinearSpectrogram.forward), :44-52 (MelScale, compress); config.py:4-19.
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

// frames per block of the n_fft kernel (consecutive frames of one utterance)
int mel_tile_frames(int n_fft);
hipError_t launch_mel(const MelArgs& a, hipStream_t s);

}  // namespace st
