"""Torch restatement of the multi-resolution discriminator of the Vocos training step (test infrastructure, not part of the
product): vocoders/vocos/models/discriminator.py:78-171, written as functions of a dict of tensors so that it runs in float64 on
the CPU (the reference of the tests) and in fp32 (the torch side of the sweep, of the trajectory test and of
tools/mrd_train_bench.py).  tests/test_mrd_cpu.py pins it to the float64 values and gradients of the REAL module
(tests/golden/mrd_grads.npz, tools/make_golden_mrd.py).  The GAN losses, the metric, the audio and the weight recipe are
tests/mpd_restatement.py's.

The spectrum is a direct DFT in matrix form -- reflect padding, frames of W samples every W / 4, the periodic hann window, then one
matrix product with cos / -sin of 2 pi (k n mod W) / W -- not torch.stft, so the reference of the native FFT shares no code
with any FFT.

Gradient comparisons are SIGN-CONSISTENT exactly as in mpd_restatement: ``forward`` writes the activation as
pre * where(sign, 1, slope), with the signs either its own or supplied ([band][layer], None entries: own).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.mpd_restatement import (gan_losses, linear_loss, loss_weights, make_audio, rel_l2, stored_elements,      # noqa: F401
                                   to_torch, weight_norm_w)

FFT_SIZES = (2048, 1024, 512)
BANDS = ((0.0, 0.1), (0.1, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0))
# (Cin, Cout, taps along F, stride along F) of band_convs.c.0 .. 4; 3 taps along the frames everywhere; conv_post: 32 -> 1, (3, 3)
LAYERS = ((2, 32, 9, 1), (32, 32, 9, 2), (32, 32, 9, 2), (32, 32, 9, 2), (32, 32, 3, 1))
SLOPE = 0.1

# fixture cases (tools/make_golden_mrd.py)
LINEAR_CASES = {"linear_w32": (32, 2, 97, 101, 102), "linear_w128": (128, 3, 331, 111, 112)}      # window, B, T, weight seed, audio seed
TRAIN_STEP = dict(B=2, T=2100, seeds=(201, 202, 203, 204, 205, 206, 207, 208))                      # first seed without a sign flip


def stored(index, g, seed):
    """What the fixture keeps of a tensor: all of it up to 512 elements, else the first 256 of mpd_restatement's sampled elements
    (234 parameters and 105 feature maps have to fit the fixture's size limit)."""
    kept = stored_elements(index, g, seed)
    return kept if np.size(g) <= 512 else kept[:256]


def band_ranges(W, bands=BANDS):
    n_fft = W // 2 + 1
    return [(int(b[0] * n_fft), int(b[1] * n_fft)) for b in bands]


def conv_names(c, i, prefix=""):
    """(g, v, bias) state-dict names of band_convs.c.i (i < 5) or conv_post (i = 5)."""
    base = prefix + (f"band_convs.{c}.{i}." if i < 5 else "conv_post.")
    return base + "parametrizations.weight.original0", base + "parametrizations.weight.original1", base + "bias"


def make_dr_state_dict(seed, prefix=""):
    """One DiscriminatorR by mpd_restatement's recipe: v ~ N(0, 1 / (Cin taps)), g = ||v|| U(0.5, 1.5) (so g != ||v||: both
    weight-norm gradients are live), bias ~ U(-0.1, 0.1); float32, the reference's names, shapes and order."""
    rng = np.random.default_rng(seed)
    sd = {}
    convs = [(c, i) + LAYERS[i] for c in range(5) for i in range(5)] + [(0, 5, 32, 1, 3, 1)]
    for c, i, cin, cout, kw, _ in convs:
        v = rng.standard_normal((cout, cin, 3, kw)) / np.sqrt(cin * 3 * kw)
        g = np.sqrt((v ** 2).sum(axis=(1, 2, 3), keepdims=True)) * rng.uniform(0.5, 1.5, (cout, 1, 1, 1))
        gn, vn, bn = conv_names(c, i, prefix)
        sd[bn] = rng.uniform(-0.1, 0.1, cout).astype(np.float32)
        sd[gn] = g.astype(np.float32)
        sd[vn] = v.astype(np.float32)
    return sd


def make_mrd_state_dict(seed, fft_sizes=FFT_SIZES):
    sd = {}
    for k in range(len(fft_sizes)):
        sd.update(make_dr_state_dict(seed + 17 * k, f"discriminators.{k}."))
    return sd


def with_windows(sd, fft_sizes=None):
    """sd plus the ``spec_fn.window`` buffers a real checkpoint carries (torchaudio's Spectrogram registers its window persistent):
    of one DiscriminatorR(fft_sizes) when fft_sizes is an int, else of the MultiResolutionDiscriminator, in state_dict order."""
    if isinstance(fft_sizes, int):
        return {"spec_fn.window": torch.hann_window(fft_sizes).numpy(), **sd}
    out = {}
    for k, W in enumerate(FFT_SIZES if fft_sizes is None else fft_sizes):
        out[f"discriminators.{k}.spec_fn.window"] = torch.hann_window(W).numpy()
        out.update({n: v for n, v in sd.items() if n.startswith(f"discriminators.{k}.")})
    return out


_DFT = {}


def dft_matrices(W, dtype, device):
    """(window (W), cos (W, W / 2 + 1), -sin (W, W / 2 + 1)): the matrices computed in float64 with the angle reduced mod W, then
    cast; the window is torchaudio's buffer, torch.hann_window(W) in fp32 (the module's .double() casts those fp32 values)."""
    key = (W, dtype, str(device))
    if key not in _DFT:
        n = torch.arange(W, dtype=torch.int64)
        k = torch.arange(W // 2 + 1, dtype=torch.int64)
        ang = ((n[:, None] * k[None, :]) % W).double() * (2 * math.pi / W)
        win = torch.hann_window(W, dtype=torch.float32)
        _DFT[key] = tuple(t.to(device=device, dtype=dtype) for t in (win, torch.cos(ang), -torch.sin(ang)))
    return _DFT[key]


def spectrum(x, W):
    """x (B, 1, T) -> (B, 2, frames, W / 2 + 1): Re and Im of Spectrogram(n_fft=W, hop_length=W // 4, power=None) in the conv layout."""
    win, cs, sn = dft_matrices(W, x.dtype, x.device)
    xp = F.pad(x, (W // 2, W // 2), mode="reflect").squeeze(1)
    fr = xp.unfold(-1, W, W // 4) * win
    return torch.stack([fr @ cs, fr @ sn], dim=1)


class Out:
    """fmaps: the 21 returned maps; signs: pre > 0 of [band][layer 0..4] (own); spec: the spectrum; acts0: layer 0's post-activation
    per band (no returned map shows it)."""
    def __init__(self, fmaps, signs, spec, acts0):
        self.fmaps, self.signs, self.spec, self.acts0 = fmaps, signs, spec, acts0


def forward(sd, x, W, slope=SLOPE, signs=None, prefix="", bands=BANDS):
    """DiscriminatorR.forward on a dict of tensors.  x (B, 1, T).  signs: None (own) or [band][layer] bool tensors (None: own)."""
    spec = spectrum(x, W)
    fmaps, own, last, acts0 = [], [], [], []
    one = torch.ones((), dtype=x.dtype, device=x.device)
    sl = torch.full((), slope, dtype=x.dtype, device=x.device)
    for c, (lo, hi) in enumerate(band_ranges(W, bands)):
        h = spec[..., lo:hi]
        own.append([])
        for i, (_, _, kw, st) in enumerate(LAYERS):
            gn, vn, bn = conv_names(c, i, prefix)
            pre = F.conv2d(h, weight_norm_w(sd[vn], sd[gn]), sd[bn], stride=(1, st), padding=(1, kw // 2))
            own[-1].append(pre.detach() > 0)
            sg = own[-1][-1] if signs is None or signs[c] is None or signs[c][i] is None else signs[c][i]
            h = pre * torch.where(sg, one, sl)
            if i > 0:
                fmaps.append(h)
            else:
                acts0.append(h.detach())
        last.append(h)
    gn, vn, bn = conv_names(0, 5, prefix)
    fmaps.append(F.conv2d(torch.cat(last, dim=-1), weight_norm_w(sd[vn], sd[gn]), sd[bn], stride=1, padding=(1, 1)))
    return Out(fmaps, own, spec, acts0)


def mrd_forward(sd, y, y_hat, slope=SLOPE, fft_sizes=FFT_SIZES, signs=None):
    """MultiResolutionDiscriminator.forward: per resolution the Out of cat([y, y_hat]) (its first half is the real signal's)."""
    x = torch.cat([y, y_hat], dim=0)
    return [forward(sd, x, W, slope, None if signs is None else signs[k], f"discriminators.{k}.") for k, W in enumerate(fft_sizes)]
