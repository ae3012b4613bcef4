"""Torch restatement of the MelStyleEncoder / DurationPredictor forwards (models/reference_encoder.py:22-93,
models/duration_predictor.py:5-37) over a parameter dict, with injectable dropout factors (test infrastructure).

``drop`` maps a site to its factor tensor (keep / (1 - p) or 0), laid out as the native kernels index the site:
  style: "spec0" / "spec1" (B, hidden, T) after each Mish, "glu0" / "glu1" (B, hidden, T) on the gated product,
         "attn" (B, heads, T, T) on the attention probabilities;
  dp:    "norm1" / "norm2" (B, filter, T) after each LayerNorm.
A missing site means no dropout (eval mode).  Also: the seeded loss projections and the fixture cases of
tests/golden/style_dp_grads.npz (tools/make_golden_style_dp_grads.py), and the numpy rebuild of the native keep masks."""
import numpy as np
import torch
import torch.nn.functional as F

# name -> (B, T, lengths or None, input seed)
STYLE_GRAD_CASES = {"se_b1_t1": (1, 1, None, 41), "se_b3_t37": (3, 37, [37, 20, 5], 42), "se_b2_t333": (2, 333, [333, 70], 43)}
DP_GRAD_CASES = {"dp_b3_t37": (3, 37, [37, 25, 9], 51), "dp_b2_t200": (2, 200, [200, 131], 52)}
STYLE_SALTS = {"spec0": 64, "spec1": 65, "glu0": 66, "glu1": 67, "attn": 68}
DP_SALTS = {"norm1": 72, "norm2": 73}


def loss_weights(shape, seed):
    rng = np.random.Generator(np.random.PCG64(seed + 5000))
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def sample_index(numel, seed, k=512):
    """Fixed element indices of a large gradient stored in the fixture (flat, sorted, unique)."""
    rng = np.random.Generator(np.random.PCG64(seed + 9000))
    return np.unique(rng.integers(0, numel, size=min(k, numel)))


def style_forward(sd, x, x_mask=None, drop=None, n_head=2):
    drop = drop or {}
    f = lambda site, t: t * drop[site] if site in drop else t      # noqa: E731
    B, _, T = x.shape
    h = F.mish(F.linear(x.transpose(1, 2), sd["spectral.0.weight"], sd["spectral.0.bias"])).transpose(1, 2)
    h = f("spec0", h)
    h = F.mish(F.linear(h.transpose(1, 2), sd["spectral.3.weight"], sd["spectral.3.bias"])).transpose(1, 2)
    h = f("spec1", h)
    Hd = h.shape[1]
    for i in range(2):
        w = sd[f"temporal.{i}.conv1.weight"]
        u = F.conv1d(h, w, sd[f"temporal.{i}.conv1.bias"], padding=w.shape[2] // 2)
        h = h + f(f"glu{i}", u[:, :Hd] * torch.sigmoid(u[:, Hd:]))
    ht = h.transpose(1, 2)
    qkv = F.linear(ht, sd["slf_attn.in_proj_weight"], sd["slf_attn.in_proj_bias"])
    q, k, v = (t.reshape(B, T, n_head, Hd // n_head).transpose(1, 2) for t in qkv.split(Hd, dim=2))
    s = (q * (Hd // n_head) ** -0.5) @ k.transpose(2, 3)
    valid = None
    if x_mask is not None:
        valid = x_mask.reshape(B, T) != 0
        s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    p = f("attn", torch.softmax(s, dim=-1))
    o = (p @ v).transpose(1, 2).reshape(B, T, Hd)
    o = F.linear(o, sd["slf_attn.out_proj.weight"], sd["slf_attn.out_proj.bias"])
    o = F.linear(o, sd["fc.weight"], sd["fc.bias"])
    if valid is None:
        return o.mean(dim=1)
    return (o * valid[:, :, None]).sum(dim=1) / valid.sum(dim=1, keepdim=True)


def dp_forward(sd, x, x_mask, g, drop=None):
    drop = drop or {}
    f = lambda site, t: t * drop[site] if site in drop else t      # noqa: E731
    x = x.detach() + F.conv1d(g.detach().unsqueeze(2), sd["cond.weight"], sd["cond.bias"])
    k = sd["conv1.weight"].shape[2]
    x = torch.relu(F.conv1d(x * x_mask, sd["conv1.weight"], sd["conv1.bias"], padding=k // 2))
    x = f("norm1", F.layer_norm(x.transpose(1, 2), (x.shape[1],), sd["norm1.weight"], sd["norm1.bias"]).transpose(1, 2))
    x = torch.relu(F.conv1d(x * x_mask, sd["conv2.weight"], sd["conv2.bias"], padding=k // 2))
    x = f("norm2", F.layer_norm(x.transpose(1, 2), (x.shape[1],), sd["norm2.weight"], sd["norm2.bias"]).transpose(1, 2))
    return F.conv1d(x * x_mask, sd["proj.weight"], sd["proj.bias"]) * x_mask


# ---- the native keep masks in numpy (csrc/common.h, csrc/train_kernels.hip make_drop, csrc/style_dp_drop.h)
_M = np.uint64(0xFFFFFFFF)


def _mix32(h):
    h = h ^ (h >> np.uint64(16)); h = (h * np.uint64(0x85ebca6b)) & _M
    h = h ^ (h >> np.uint64(13)); h = (h * np.uint64(0xc2b2ae35)) & _M
    return h ^ (h >> np.uint64(16))


def _seed_words(seed, salt):
    s64 = (seed * 0x100000001B3 + (salt + 1) * 0xD6E8FEB86659FD93) % (1 << 64)
    return np.uint64(s64 & 0xFFFFFFFF), np.uint64(s64 >> 32)


def _keep(h, odd, p):
    thresh = min(max(int(p * 65536.0 + 0.5), 1), 65535)
    half = np.where(odd, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return np.where(half >= np.uint64(thresh), np.float32(1.0 / (1.0 - p)), np.float32(0.0)).astype(np.float32)


def drop_elem(seed, salt, p, shape):
    """Element site: factor of element i of the C-contiguous tensor `shape`."""
    lo, hi = _seed_words(seed, salt)
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
    h = _mix32(((lo ^ (((idx >> np.uint64(1)) * np.uint64(0x9E3779B1)) & _M)) + hi) & _M)
    return torch.from_numpy(_keep(h, (idx & np.uint64(1)) == 1, p).reshape(shape))


def drop_attn(seed, salt, p, B, H, T):
    """Attention site: factor of (item, head, query, key), row = (item * H + head) * T + query."""
    lo, hi = _seed_words(seed, salt)
    row = np.arange(B * H * T, dtype=np.uint64)[:, None]
    key = np.arange(T, dtype=np.uint64)[None, :]
    rh = _mix32(lo ^ ((row * np.uint64(0x9E3779B1)) & _M))
    ch = _mix32(hi ^ (((key >> np.uint64(1)) * np.uint64(0x85ebca77)) & _M))
    x = ((rh ^ ch) * np.uint64(0x9E3779B1)) & _M
    x = x ^ (x >> np.uint64(15))
    return torch.from_numpy(_keep(x, (key & np.uint64(1)) == 1, p).reshape(B, H, T, T))


def style_drops(seed, p, B, hidden, T, H=2):
    d = {s: drop_elem(seed, STYLE_SALTS[s], p, (B, hidden, T)) for s in ("spec0", "spec1", "glu0", "glu1")}
    d["attn"] = drop_attn(seed, STYLE_SALTS["attn"], p, B, H, T)
    return d


def dp_drops(seed, p, B, filt, T):
    return {s: drop_elem(seed, DP_SALTS[s], p, (B, filt, T)) for s in ("norm1", "norm2")}
