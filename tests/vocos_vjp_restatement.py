"""Float64 numpy restatement of the Vocos generator's backward (test infrastructure, not part of the product): the VJP of
``oracle.vocos_oracle.vocos_forward`` (vocoders/vocos/models/backbone.py:50-56, module.py:33-46, head.py:39-72,93-117) from
d audio to every parameter and to the mel, written out by hand -- the formulas the native backward implements (DESIGN.md,
"Vocos training").  tests/test_vocos_backward_cpu.py pins it to the float64 gradients of the REAL module under torch autograd
(tests/golden/vocos_grads.npz, tools/make_golden_vocos_grads.py); the GPU tests use it at shapes the fixture lacks.

The contractions over the frames go through ``optimize=True`` (BLAS): the reference of a 4100-frame case takes seconds.

Also here: the fixtures' cases, its sampled-element rule, and ``torch_vocos``, a functional torch statement of the same
forward on a dict of tensors, which the GPU trajectory test and tools/vocos_train_bench.py differentiate with torch autograd.
"""
import numpy as np
from scipy.special import erf

from oracle import vocos_oracle as vo

FULL_MAX = 512        # tensors up to this many elements are stored whole (every width-C vector), larger ones as 512 sampled elements

# fixture cases (tools/make_golden_vocos_grads.py): name -> (config fields, B, T, weight seed, mel seed, loss)
CASES = {
    "preset_linear": (dict(), 2, 40, 11, 12, "linear"),
    "small_linear": (dict(input_channels=64, intermediate_dim=256, num_layers=2), 3, 7, 21, 22, "linear"),
    "preset_mel_loss": (dict(), 2, 16, 31, 32, "mel_loss"),
}
# cases above 128 frames per batch (tests/golden/vocos_grads_frames.npz): the split-K weight gradients take several planes.  The
# same layout, except that d mel and the audio are stored as FRAMES_SAMPLE sampled elements too (sampled())
FRAME_CASES = {
    "R1100": (dict(input_channels=64, intermediate_dim=256, num_layers=2), 25, 44, 41, 42, "linear"),
    "preset_R260": (dict(), 4, 65, 41, 42, "linear"),
}
FRAMES_SAMPLE = 4096


def loss_weights(shape, seed):
    """W of the loss sum(audio * W)."""
    rng = np.random.Generator(np.random.PCG64(seed + 5000))
    return rng.standard_normal(shape).astype(np.float32)


def sample_index(numel, seed, k=512):
    """Fixed element indices of a large gradient stored in the fixture (flat, sorted, unique)."""
    rng = np.random.Generator(np.random.PCG64(seed + 9000))
    return np.unique(rng.integers(0, numel, size=min(k, numel)))


def stored_elements(name_index, g, seed):
    """What the fixture keeps of gradient ``g``: all of it up to FULL_MAX elements, else the sampled elements."""
    g = np.asarray(g).reshape(-1)
    return g if g.size <= FULL_MAX else g[sample_index(g.size, seed + name_index)]


def sampled(x, seed, which):
    """What the frames fixture keeps of d mel (which = 0) and of the audio (which = 1): FRAMES_SAMPLE fixed sampled elements."""
    x = np.asarray(x).reshape(-1)
    rng = np.random.Generator(np.random.PCG64(seed + 9500 + which))
    return x[np.sort(rng.choice(x.size, size=min(FRAMES_SAMPLE, x.size), replace=False))]


def param_names(sd):
    """Names of the trainable parameters (everything but the window buffer), sorted as the fixture stores them."""
    return sorted(k for k in sd if k != "head.istft.window")


# ---- forward that keeps what the backward needs ---------------------------------------------------------------------
def _ln_fwd(x, w, b, eps=1e-6):
    mu = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps)
    xhat = (x - mu) * rstd
    return xhat * w + b, (xhat, rstd)


def _ln_bwd(dy, kept, w):
    xhat, rstd = kept
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdims=True) - xhat * (g * xhat).mean(-1, keepdims=True))
    red = tuple(range(dy.ndim - 1))
    return dx, (dy * xhat).sum(red), dy.sum(red)


def _cols(x, K=7):
    T = x.shape[2]
    xp = np.pad(x, ((0, 0), (0, 0), (K // 2, K // 2)))
    return np.stack([xp[:, :, j:j + T] for j in range(K)], axis=-1)          # (B, C, T, K): x[b][c][t + j - 3]


def _cols_T(dcols):
    """Transpose of _cols: dx[b][c][t] = sum_j dcols[b][c][t - j + 3][j]."""
    B, C, T, K = dcols.shape
    dxp = np.zeros((B, C, T + K - 1), dcols.dtype)
    for j in range(K):
        dxp[:, :, j:j + T] += dcols[..., j]
    return dxp[:, :, K // 2:K // 2 + T]


def forward(sd, mel, cfg=vo.VocosConfig):
    """-> (audio (B, T * hop) float64, kept).  The same arithmetic as vocos_oracle.vocos_forward(dtype=float64)."""
    g = lambda k: sd[k].astype(np.float64)      # noqa: E731
    kept = {"mel_cols": _cols(mel.astype(np.float64))}
    e0 = np.einsum("bctk,ock->bot", kept["mel_cols"], g("backbone.embed.weight"), optimize=True) + g("backbone.embed.bias")[None, :, None]
    x, kept["ln0"] = _ln_fwd(e0.transpose(0, 2, 1), g("backbone.norm.weight"), g("backbone.norm.bias"))
    x = x.transpose(0, 2, 1)                                                  # (B, C, T)
    for i in range(cfg.num_layers):
        p = f"backbone.convnext.{i}."
        k = {"x_cols": _cols(x)}
        z = np.einsum("bctk,ck->bct", k["x_cols"], g(p + "dwconv.weight")[:, 0]) + g(p + "dwconv.bias")[None, :, None]
        h, k["ln"] = _ln_fwd(z.transpose(0, 2, 1), g(p + "norm.weight"), g(p + "norm.bias"))      # (B, T, C)
        k["h"] = h
        k["u"] = h @ g(p + "pwconv1.weight").T + g(p + "pwconv1.bias")
        k["g"] = vo.gelu(k["u"])
        k["y2"] = k["g"] @ g(p + "pwconv2.weight").T + g(p + "pwconv2.bias")
        x = x + (g(p + "gamma") * k["y2"]).transpose(0, 2, 1)
        kept[i] = k
    hf, kept["lnf"] = _ln_fwd(x.transpose(0, 2, 1), g("backbone.final_layer_norm.weight"), g("backbone.final_layer_norm.bias"))
    kept["hf"] = hf
    o = hf @ g("head.out.weight").T + g("head.out.bias")                     # (B, T, n_fft + 2)
    kept["o"] = o
    half = o.shape[2] // 2
    a, ph = o[..., :half].transpose(0, 2, 1), o[..., half:].transpose(0, 2, 1)
    S = np.minimum(np.exp(a), 1e2) * (np.cos(ph) + 1j * np.sin(ph))
    return vo.istft_same(S, g("head.istft.window"), cfg.n_fft, cfg.hop_length), kept


# ---- backward -----------------------------------------------------------------------------------------------------------
def istft_head_backward(d_audio, o, window, n_fft, hop):
    """d loss / d o (B, T, n_fft + 2) from d loss / d audio (B, T * hop): the ISTFT (padding "same"), the complex
    spectrum S = min(exp a, 100) e^{ip} and the chunk, backwards."""
    B, T, _ = o.shape
    N, pad = n_fft, (n_fft - hop) // 2
    out_len = (T - 1) * hop + N
    env = np.zeros(out_len)
    for t in range(T):
        env[t * hop:t * hop + N] += window ** 2
    gy = np.zeros((B, out_len))
    gy[:, pad:out_len - pad] = d_audio / env[pad:out_len - pad]              # zero outside the trimmed range
    df = np.stack([window * gy[:, t * hop:t * hop + N] for t in range(T)], axis=1)      # (B, T, N): a gather
    Fq = np.fft.rfft(df, axis=-1)                                             # (B, T, N/2 + 1)
    ck = np.full(N // 2 + 1, 2.0); ck[0] = ck[-1] = 1.0
    dRe, dIm = ck / N * Fq.real, ck / N * Fq.imag
    dIm[..., 0] = 0.0; dIm[..., -1] = 0.0                                     # irfft ignores them
    half = N // 2 + 1
    a, ph = o[..., :half], o[..., half:]
    ea = np.exp(a)
    mag = np.minimum(ea, 1e2)
    da = np.where(ea <= 1e2, mag * (dRe * np.cos(ph) + dIm * np.sin(ph)), 0.0)
    dp = mag * (-dRe * np.sin(ph) + dIm * np.cos(ph))
    return np.concatenate([da, dp], axis=-1)


def gelu_grad(u):
    return 0.5 * (1.0 + erf(u / np.sqrt(2.0))) + u * np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)


def backward(sd, kept, d_audio, cfg=vo.VocosConfig):
    """-> ({parameter name: gradient in the parameter's shape}, d mel (B, input_channels, T)), float64."""
    g = lambda k: sd[k].astype(np.float64)      # noqa: E731
    G = {}
    do = istft_head_backward(d_audio.astype(np.float64), kept["o"], g("head.istft.window"), cfg.n_fft, cfg.hop_length)
    G["head.out.weight"] = np.einsum("btn,btc->nc", do, kept["hf"], optimize=True)
    G["head.out.bias"] = do.sum((0, 1))
    dhf = do @ g("head.out.weight")
    dx, G["backbone.final_layer_norm.weight"], G["backbone.final_layer_norm.bias"] = _ln_bwd(dhf, kept["lnf"], g("backbone.final_layer_norm.weight"))
    dx = dx.transpose(0, 2, 1)                                                # (B, C, T)
    for i in reversed(range(cfg.num_layers)):
        p = f"backbone.convnext.{i}."
        k = kept[i]
        dxt = dx.transpose(0, 2, 1)                                           # (B, T, C)
        G[p + "gamma"] = (dxt * k["y2"]).sum((0, 1))
        dy2 = dxt * g(p + "gamma")
        G[p + "pwconv2.weight"] = np.einsum("btc,btf->cf", dy2, k["g"], optimize=True)
        G[p + "pwconv2.bias"] = dy2.sum((0, 1))
        du = (dy2 @ g(p + "pwconv2.weight")) * gelu_grad(k["u"])
        G[p + "pwconv1.weight"] = np.einsum("btf,btc->fc", du, k["h"], optimize=True)
        G[p + "pwconv1.bias"] = du.sum((0, 1))
        dh = du @ g(p + "pwconv1.weight")
        dz, G[p + "norm.weight"], G[p + "norm.bias"] = _ln_bwd(dh, k["ln"], g(p + "norm.weight"))
        dz = dz.transpose(0, 2, 1)                                            # (B, C, T)
        G[p + "dwconv.weight"] = np.einsum("bct,bctk->ck", dz, k["x_cols"])[:, None, :]
        G[p + "dwconv.bias"] = dz.sum((0, 2))
        dx = dx + _cols_T(dz[..., None] * g(p + "dwconv.weight")[None, :, 0, None, :])
    de0, G["backbone.norm.weight"], G["backbone.norm.bias"] = _ln_bwd(dx.transpose(0, 2, 1), kept["ln0"], g("backbone.norm.weight"))
    de0 = de0.transpose(0, 2, 1)
    G["backbone.embed.weight"] = np.einsum("bot,bctk->ock", de0, kept["mel_cols"], optimize=True)
    G["backbone.embed.bias"] = de0.sum((0, 2))
    dmel = _cols_T(np.einsum("bot,ock->bctk", de0, g("backbone.embed.weight"), optimize=True))
    return G, dmel


# ---- the same forward as a torch function of a dict of tensors (for torch autograd on any device / dtype) ------------
def torch_vocos(p, mel, num_layers, n_fft=2048, hop=512):
    import torch
    import torch.nn.functional as F
    C = p["backbone.embed.weight"].shape[0]
    x = F.conv1d(mel, p["backbone.embed.weight"], p["backbone.embed.bias"], padding=3)
    x = F.layer_norm(x.transpose(1, 2), (C,), p["backbone.norm.weight"], p["backbone.norm.bias"], 1e-6).transpose(1, 2)
    for i in range(num_layers):
        q = f"backbone.convnext.{i}."
        h = F.conv1d(x, p[q + "dwconv.weight"], p[q + "dwconv.bias"], padding=3, groups=C).transpose(1, 2)
        h = F.layer_norm(h, (C,), p[q + "norm.weight"], p[q + "norm.bias"], 1e-6)
        h = F.linear(F.gelu(F.linear(h, p[q + "pwconv1.weight"], p[q + "pwconv1.bias"])), p[q + "pwconv2.weight"], p[q + "pwconv2.bias"])
        x = x + (p[q + "gamma"] * h).transpose(1, 2)
    x = F.layer_norm(x.transpose(1, 2), (C,), p["backbone.final_layer_norm.weight"], p["backbone.final_layer_norm.bias"], 1e-6)
    o = F.linear(x, p["head.out.weight"], p["head.out.bias"]).transpose(1, 2)
    mag, ph = o.chunk(2, dim=1)
    mag = torch.clip(torch.exp(mag), max=1e2)
    S = mag * (torch.cos(ph) + 1j * torch.sin(ph))
    win = p["head.istft.window"]
    T, pad = S.shape[2], (n_fft - hop) // 2
    fr = torch.fft.irfft(S, n_fft, dim=1, norm="backward") * win[None, :, None]
    out_len = (T - 1) * hop + n_fft
    y = F.fold(fr, output_size=(1, out_len), kernel_size=(1, n_fft), stride=(1, hop))[:, 0, 0, pad:out_len - pad]
    env = F.fold(win.square().expand(1, T, -1).transpose(1, 2), output_size=(1, out_len), kernel_size=(1, n_fft),
                 stride=(1, hop)).reshape(-1)[pad:out_len - pad]
    return y / env
