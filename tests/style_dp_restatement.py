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


def grad_digest(grads, seed, full_max=4096):
    """What tests/golden/style_dp_configs.npz keeps of a case's gradients {name: array}: the sorted names, per name the
    float64 norm and max |g|, and two flat float arrays in name order: every tensor of at most full_max elements whole, and
    sample_index(numel, seed + position) of each larger one."""
    names = sorted(grads)
    flat = [np.asarray(grads[n]).reshape(-1) for n in names]
    full = [g for g in flat if g.size <= full_max]
    samp = [g[sample_index(g.size, seed + i)] for i, g in enumerate(flat) if g.size > full_max]
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.float32)      # noqa: E731
    return dict(names=np.array(names), norms=np.array([float(np.linalg.norm(g.astype(np.float64))) for g in flat]),
                absmax=np.array([float(np.abs(g).max()) for g in flat]), full=cat(full), sample=cat(samp),
                owner_full=np.concatenate([np.full(g.size, i) for i, g in enumerate(flat) if g.size <= full_max] or [np.zeros(0, int)]),
                owner_sample=np.concatenate([np.full(sample_index(g.size, seed + i).size, i) for i, g in enumerate(flat) if g.size > full_max]
                                            or [np.zeros(0, int)]))


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


def dp_forward(sd, x, x_mask, g, drop=None, return_pre=False):
    """return_pre: also the two ReLU pre-activations (conv1's and conv2's outputs), for the tests that check that none of
    them is close enough to 0 for a rounding difference to flip it."""
    drop = drop or {}
    f = lambda site, t: t * drop[site] if site in drop else t      # noqa: E731
    x = x.detach() + F.conv1d(g.detach().unsqueeze(2), sd["cond.weight"], sd["cond.bias"])
    k = sd["conv1.weight"].shape[2]
    pre1 = F.conv1d(x * x_mask, sd["conv1.weight"], sd["conv1.bias"], padding=k // 2)
    x = torch.relu(pre1)
    x = f("norm1", F.layer_norm(x.transpose(1, 2), (x.shape[1],), sd["norm1.weight"], sd["norm1.bias"]).transpose(1, 2))
    pre2 = F.conv1d(x * x_mask, sd["conv2.weight"], sd["conv2.bias"], padding=k // 2)
    x = torch.relu(pre2)
    x = f("norm2", F.layer_norm(x.transpose(1, 2), (x.shape[1],), sd["norm2.weight"], sd["norm2.bias"]).transpose(1, 2))
    logw = F.conv1d(x * x_mask, sd["proj.weight"], sd["proj.bias"]) * x_mask
    return (logw, (pre1, pre2)) if return_pre else logw


def kink_margin(pre64, pre32, x_mask):
    """(min |float64 pre-activation|, max |fp32 - float64| pre-activation) over both ReLU sites, valid tokens only: a padded
    token's activations are multiplied by x_mask before anything reads them, so a flip there changes nothing."""
    v = (torch.as_tensor(x_mask) != 0).reshape(x_mask.shape[0], 1, -1).cpu()
    lo, diff = float("inf"), 0.0
    for a, b in zip(pre64, pre32):
        a = a.detach().double(); b = b.detach().double()
        lo = min(lo, float(a.abs().masked_fill(~v, float("inf")).min()))
        diff = max(diff, float((a - b).abs().masked_fill(~v, 0.0).max()))
    return lo, diff


# ---- the float64 runs the tests compare with: output, loss against the seeded projection, parameter gradients
def _as(sd, dtype):
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def run_style(sd, y, mask, seed, n_head=2, drop=None, dtype=torch.float64):
    """(c, loss, {name: gradient}) of style_forward in `dtype` on the CPU; y / mask numpy or tensors, mask may be None."""
    p = _as(sd, dtype)
    t = lambda a: None if a is None else torch.as_tensor(a).detach().cpu().to(dtype)      # noqa: E731
    c = style_forward(p, t(y), t(mask), drop={k: v.to(dtype) for k, v in (drop or {}).items()}, n_head=n_head)
    loss = (c * loss_weights(tuple(c.shape), seed).to(dtype)).sum()
    loss.backward()
    return c.detach().numpy(), float(loss.detach()), {k: v.grad.numpy() for k, v in p.items()}


def run_dp(sd, x, mask, g, seed, drop=None, dtype=torch.float64):
    """(logw, loss, {name: gradient}, (pre1, pre2)) of dp_forward in `dtype` on the CPU."""
    p = _as(sd, dtype)
    t = lambda a: torch.as_tensor(a).detach().cpu().to(dtype)      # noqa: E731
    logw, pre = dp_forward(p, t(x), t(mask), t(g), drop={k: v.to(dtype) for k, v in (drop or {}).items()}, return_pre=True)
    loss = (logw * loss_weights(tuple(logw.shape), seed).to(dtype)).sum()
    loss.backward()
    return logw.detach().numpy(), float(loss.detach()), {k: v.grad.numpy() for k, v in p.items()}, tuple(a.detach() for a in pre)


def digest_errors(ref, grads, seed):
    """{name: (max |g - ref| / max |ref| over the kept elements, |norm - ref norm| / ref norm)} of gradients {name: array}
    against a stored or computed grad_digest `ref` (a mapping with names, norms, absmax, full, sample)."""
    d = grad_digest(grads, seed)
    names = [str(n) for n in ref["names"]]
    assert [str(n) for n in d["names"]] == names, (d["names"], names)
    assert d["full"].shape == ref["full"].shape and d["sample"].shape == ref["sample"].shape
    err = np.zeros(len(names))
    for part in ("full", "sample"):
        diff = np.abs(d[part].astype(np.float64) - np.asarray(ref[part], dtype=np.float64))
        np.maximum.at(err, d["owner_" + part], diff)
    scale = np.maximum(np.asarray(ref["absmax"], dtype=np.float64), 1e-30)
    nref = np.asarray(ref["norms"], dtype=np.float64)
    return {n: (float(err[i] / scale[i]), float(abs(d["norms"][i] - nref[i]) / max(nref[i], 1e-30))) for i, n in enumerate(names)}


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
