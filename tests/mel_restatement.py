"""Float64 numpy restatement of the reference's feature front end (utils/audio.py:19-26,50-52 with center=False): reflect
padding, framing, window, rfft, magnitude, mel projection, log -- for checks beyond tests/golden/mel_outputs.npz.

    mag = linear(wave, window, n_fft, hop, pad)            # wave (B, L) -> (B, n_fft // 2 + 1, frames)
    mel = log_mel(wave, window, fb, n_fft, hop, pad)       # fb (n_fft // 2 + 1, n_mels) -> (B, n_mels, frames)

numpy's "reflect" padding is torch's: the edge sample is not repeated.
"""
import numpy as np


def frames(L, n_fft, hop, pad):
    return 1 + (L + 2 * pad - n_fft) // hop


def linear(wave, window, n_fft, hop, pad):
    x = np.asarray(wave, np.float64)
    if x.ndim == 1:
        x = x[None]
    B, L = x.shape
    assert L > pad and L + 2 * pad >= n_fft
    xp = np.pad(x, ((0, 0), (pad, pad)), mode="reflect")
    T = frames(L, n_fft, hop, pad)
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None]
    fr = xp[:, idx] * np.asarray(window, np.float64)[None, None]          # (B, T, n_fft)
    X = np.fft.rfft(fr, axis=-1)
    return np.sqrt(X.real ** 2 + X.imag ** 2 + 1e-6).transpose(0, 2, 1)    # (B, bins, T)


def log_mel(wave, window, fb, n_fft, hop, pad):
    mag = linear(wave, window, n_fft, hop, pad)
    mel = np.einsum("km,bkt->bmt", np.asarray(fb, np.float64), mag)
    return np.log(np.maximum(mel, 1e-5))
