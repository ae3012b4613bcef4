"""Float64 numpy restatement of the spectrogram's backward (the vector-Jacobian product of tests/mel_restatement.py), step by step
as st_mel_backward computes it (stabletts_amd/csrc/audio_launch.h):

    1. dmel = g / mel where mel >= 1e-5, else 0            (linear spectrogram: dmag = g)
    2. dmag = fb dmel
    3. G = dmag X / mag
    4. df_t = N irfft(C),  C_0 = Re G_0, C_{N/2} = Re G_{N/2}, C_k = G_k / 2 otherwise
    5. dx = gather(w df_t): per sample, its direct padded position, then the left reflection, then the right, each by ascending t

    dx = vjp(wave, window, fb, n_fft, hop, pad, g)          # fb None: the linear spectrogram; g of the output's shape
    dx = gather(wdf, L, hop, pad)                           # step 5 by index inversion; scatter() is the brute-force form
    y = torch_forward(x, window, fb, n_fft, hop, pad)       # the reference's forward in torch (any dtype / device, autograd)
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import mel_restatement as mr


def _frames(x, window, n_fft, hop, pad):
    B, L = x.shape
    xp = np.pad(x, ((0, 0), (pad, pad)), mode="reflect")
    T = mr.frames(L, n_fft, hop, pad)
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None]
    return xp[:, idx] * np.asarray(window, np.float64)[None, None]           # (B, T, n_fft)


def frame_grads(wave, window, fb, n_fft, hop, pad, g):
    """Steps 1-4: w * df_t, (B, T, n_fft)."""
    x = np.asarray(wave, np.float64)
    if x.ndim == 1:
        x = x[None]
    X = np.fft.rfft(_frames(x, window, n_fft, hop, pad), axis=-1)            # (B, T, bins)
    mag = np.sqrt(X.real ** 2 + X.imag ** 2 + 1e-6)
    g = np.asarray(g, np.float64).transpose(0, 2, 1)                          # (B, T, rows)
    if fb is None:
        dmag = g
    else:
        fb = np.asarray(fb, np.float64)
        mel = mag @ fb
        dmel = np.where(mel >= 1e-5, g / mel, 0.0)
        dmag = dmel @ fb.T
    G = dmag * X / mag
    C = G / 2
    C[..., 0] = G[..., 0].real
    C[..., -1] = G[..., -1].real
    df = n_fft * np.fft.irfft(C, n=n_fft, axis=-1)
    return df * np.asarray(window, np.float64)[None, None]


def gather(wdf, L, hop, pad):
    """Step 5 by index inversion, in the kernel's order: dx (B, L)."""
    B, T, N = wdf.shape
    s = np.arange(L)
    dx = np.zeros((B, L))

    def add(q, valid):
        tlo = np.where(q < N, 0, (q - N + hop) // hop)
        thi = np.minimum(q // hop, T - 1)
        for j in range(-(-N // hop) + 1):
            t = tlo + j
            ok = valid & (t <= thi)
            tt, n = np.where(ok, t, 0), np.where(ok, q - t * hop, 0)
            dx[:] += np.where(ok[None], wdf[:, tt, n], 0.0)

    add(s + pad, np.ones(L, bool))
    add(np.where((s >= 1) & (s <= pad), pad - s, 0), (s >= 1) & (s <= pad))
    add(np.where(s <= L - 2, 2 * (L - 1) - s + pad, 0), s <= L - 2)
    return dx


def scatter(wdf, L, hop, pad):
    """Step 5 by brute force: every frame element added to the sample its padded position reads."""
    B, T, N = wdf.shape
    q = np.arange(T)[:, None] * hop + np.arange(N)[None] - pad
    q = np.where(q < 0, -q, q)
    q = np.where(q >= L, 2 * (L - 1) - q, q)
    dx = np.zeros((B, L))
    for b in range(B):
        np.add.at(dx[b], q.reshape(-1), wdf[b].reshape(-1))
    return dx


def vjp(wave, window, fb, n_fft, hop, pad, g):
    x = np.asarray(wave, np.float64)
    if x.ndim == 1:
        x = x[None]
    return gather(frame_grads(x, window, fb, n_fft, hop, pad, g), x.shape[1], hop, pad)


def torch_forward(x, window, fb, n_fft, hop, pad):
    """utils/audio.py:19-26,50-52 (center=False) in torch: x (B, L) -> log-mel (B, n_mels, frames), or the magnitude when fb
    is None."""
    xp = F.pad(x.unsqueeze(1), (pad, pad), "reflect").squeeze(1)
    spec = torch.view_as_real(torch.stft(xp, n_fft, hop, n_fft, window, False, "reflect", False, True, True))
    mag = torch.sqrt(spec.pow(2).sum(-1) + 1e-6)
    if fb is None:
        return mag
    return torch.log(torch.clamp(torch.matmul(mag.transpose(-1, -2), fb).transpose(-1, -2), min=1e-5))
