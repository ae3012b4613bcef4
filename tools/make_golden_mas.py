"""Generates tests/golden/mas_outputs.npz from the REAL reference monotonic_align (monotonic_align/__init__.py +
core.py, unmodified; numba replaced by a pass-through decorator, so the DP runs as plain Python).  Run where a checkout of
the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_mas.py

Cases (each stores <case>/neg_cent (B, Ty, Tx) fp32, <case>/mask (B, Ty, Tx) fp32 as models/model.py:157 builds it, and
<case>/path, the reference's maximum_path):
  ragged      random-normal neg_cent, ragged lengths
  ties        small integers: every sum is exact, so ties in the max and in the backtrack compare are common
  equal       t_x == t_y;  wide: t_x > t_y;  tx1: t_x = 1;  ty1: t_y = 1;  single: B = 1
  clear       a clear alignment: mu_x random, ground-truth durations >= 1, y = expand(mu_x) + 0.3 noise, neg_cent restated
              from models/model.py:150-155; also stores mu_x, y, x_mask, y_mask and the reference's attn, logw_, mu_y and
              prior_loss (:162-176).  Its path is asserted unchanged under +-1e-5 relative perturbations of neg_cent, so it
              tolerates a different summation order of neg_cent.
The npz is written with fixed zip timestamps, so regenerating it reproduces the committed file byte for byte.
"""
import io
import math
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mas_outputs.npz")


def _install_numba_standin():
    class _Ty:
        def __getitem__(self, item):
            return self

        def __call__(self, *a, **k):
            return self

    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (lambda f: f)
    numba.void = numba.int32 = numba.float32 = _Ty()
    sys.modules["numba"] = numba


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def masks(t_x, t_y, Tx, Ty):
    """x_mask (B, 1, Tx), y_mask (B, 1, Ty) and models/model.py:157's attn_mask squeezed to (B, Ty, Tx)."""
    x_mask = (torch.arange(Tx)[None] < torch.tensor(t_x)[:, None]).float().unsqueeze(1)
    y_mask = (torch.arange(Ty)[None] < torch.tensor(t_y)[:, None]).float().unsqueeze(1)
    attn_mask = torch.unsqueeze(x_mask, 2) * torch.unsqueeze(y_mask, -1)
    return x_mask, y_mask, attn_mask.squeeze(1)


def neg_cent_of(mu_x, y):
    """models/model.py:150-155, restated."""
    s_p_sq_r = torch.ones_like(mu_x)
    neg_cent1 = torch.sum(-0.5 * math.log(2 * math.pi) - torch.zeros_like(mu_x), [1], keepdim=True)
    neg_cent2 = torch.einsum("bdt, bds -> bts", -0.5 * (y ** 2), s_p_sq_r)
    neg_cent3 = torch.einsum("bdt, bds -> bts", y, (mu_x * s_p_sq_r))
    neg_cent4 = torch.sum(-0.5 * (mu_x ** 2) * s_p_sq_r, [1], keepdim=True)
    return neg_cent1 + neg_cent2 + neg_cent3 + neg_cent4


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref_dir, "monotonic_align")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ref_dir)
    torch.set_num_threads(1)
    _install_numba_standin()
    import monotonic_align                  # reference, unmodified
    assert os.path.dirname(monotonic_align.__file__) == os.path.join(os.path.abspath(ref_dir), "monotonic_align")
    rng = np.random.default_rng(20261015)
    out = {}

    def add(case, neg_cent, t_x, t_y):
        B, Ty, Tx = neg_cent.shape
        _, _, mask = masks(t_x, t_y, Tx, Ty)
        path = monotonic_align.maximum_path(neg_cent, mask)
        out[case + "/neg_cent"] = neg_cent.numpy()
        out[case + "/mask"] = mask.numpy()
        out[case + "/path"] = path.numpy()
        return mask, path

    def normal(*shape, scale=1.0):
        return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))

    # ragged random-normal: B = 5, Ty = 160, Tx = 48, t_x <= t_y
    t_y = [160, 131, 97, 150, 64]
    t_x = [48, 40, 30, 17, 21]
    add("ragged", normal(5, 160, 48, scale=3.0), t_x, t_y)
    # tie-heavy small integers
    ints = torch.from_numpy(rng.integers(-2, 3, size=(4, 90, 30)).astype(np.float32))
    add("ties", ints, [30, 25, 12, 30], [90, 60, 45, 30])
    add("equal", normal(3, 40, 40), [40, 23, 7], [40, 23, 7])
    add("wide", normal(3, 30, 56), [56, 45, 31], [30, 20, 9])
    add("tx1", normal(2, 50, 8), [1, 1], [50, 17])
    add("ty1", normal(2, 6, 20), [1, 9], [1, 1])
    add("single", normal(1, 77, 25), [25], [77])

    # clear alignment through models/model.py:150-176
    B, D, Tx = 3, 80, 28
    tx = [28, 21, 12]
    dur = rng.integers(1, 7, size=(B, Tx))
    dur[np.arange(Tx)[None] >= np.array(tx)[:, None]] = 0
    ty = dur.sum(1).tolist()
    Ty = max(ty)
    mu_x = normal(B, D, Tx)
    x_mask, y_mask, attn_mask = masks(tx, ty, Tx, Ty)
    mu_x = mu_x * x_mask
    idx = np.zeros((B, Ty), np.int64)
    for b in range(B):
        idx[b, :ty[b]] = np.repeat(np.arange(Tx), dur[b])
    y = torch.gather(mu_x, 2, torch.from_numpy(idx)[:, None].expand(B, D, Ty)) + 0.3 * normal(B, D, Ty)
    y = y * y_mask
    neg_cent = neg_cent_of(mu_x, y)
    attn = monotonic_align.maximum_path(neg_cent, attn_mask).unsqueeze(1).detach()
    for trial in range(4):
        sign = torch.from_numpy(rng.choice([-1.0, 1.0], size=neg_cent.shape).astype(np.float32))
        again = monotonic_align.maximum_path(neg_cent * (1 + 1e-5 * sign), attn_mask)
        assert torch.equal(again, attn.squeeze(1)), f"clear case is sensitive to 1e-5 perturbations (trial {trial})"
    logw_ = torch.log(1e-8 + attn.sum(2)) * x_mask
    a = attn.squeeze(1).transpose(1, 2)
    mu_y = torch.matmul(a.squeeze(1).transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)
    prior_loss = torch.sum(0.5 * ((y - mu_y) ** 2 + math.log(2 * math.pi)) * y_mask)
    prior_loss = prior_loss / (torch.sum(y_mask) * D)
    gt = torch.zeros(B, Ty, Tx)
    gt[torch.arange(B)[:, None], torch.arange(Ty)[None], torch.from_numpy(idx)] = 1
    gt = gt * attn_mask
    print("clear case: reference path equals the ground-truth alignment:", bool(torch.equal(gt, attn.squeeze(1))))
    for k, v in dict(mu_x=mu_x, y=y, x_mask=x_mask, y_mask=y_mask, neg_cent=neg_cent, mask=attn_mask,
                     path=attn.squeeze(1), attn=attn, logw_=logw_, mu_y=mu_y, prior_loss=prior_loss).items():
        out["clear/" + k] = v.numpy()

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    _save(OUT, out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} kB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
