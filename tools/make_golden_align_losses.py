"""Generates tests/golden/align_loss_grads.npz from the REAL reference StableTTS.forward (models/model.py:136-178, imported
unmodified) on the CPU.  Only the four submodules are replaced, by stand-ins that make the glue lines the whole computation:
the encoder returns a leaf mu_x, dp a leaf logw, ref_encoder a constant, and decoder.compute_loss returns
(sum(W * mu), None) for a stored W.  The reference's own lines then produce the alignment, logw_, both losses, mu_y and the
gradients of mu_x, logw and fake_content.  Import stand-ins for packages absent offline: numba (monotonic_align's decorator,
so the search runs as plain Python) and torchdiffeq.  Run where a checkout of the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_align_losses.py

Every case uses y = expand(mu_x) + 0.3 noise, so its alignment is clear and does not move under a different summation order
of neg_cent (asserted under +-1e-5 relative perturbations).  Per case the file holds the inputs (x_lengths, y_lengths, mu_x,
logw, y, W, fake_content), keep (the cfg mask the forward drew), durations (attn.sum over frames, int32), attn (B, Tx, Ty)
uint8, the fp32 results (dur_loss, prior_loss, diff_loss, mu_y, mu_y_masked, grad_mu_x, grad_logw, grad_fake_content) and,
with the suffix _f64, the losses and gradients of a float64 run of the same lines on the same inputs and the same mask.
Cases:
  ragged         B = 4, M = 80, Tx = 37, Ty = 300: ragged lengths, one item at full length, one token of 270 frames, many of
                 1 frame, a mixed cfg mask
  wide           B = 3, M = 100, one item with t_x > t_y (tokens of 0 frames), mixed cfg mask
  edges_dropped  B = 3: one item with t_x = 1, one with t_y = 1, one with every token and frame valid; every item dropped
  edges_kept     the same inputs, every item kept
W and the noise are multiples of 1/4 and 1/64: they compress well.  The npz is written with fixed zip timestamps, so
regenerating it reproduces the committed file byte for byte.
"""
import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "align_loss_grads.npz")
GIN = 8


def _install_standins():
    class _Ty:
        def __getitem__(self, item):
            return self

        def __call__(self, *a, **k):
            return self

    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (lambda f: f)
    numba.void = numba.int32 = numba.float32 = _Ty()
    tde = types.ModuleType("torchdiffeq")
    tde.odeint = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("stand-in"))
    sys.modules["numba"] = numba
    sys.modules["torchdiffeq"] = tde


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


class _Encoder(torch.nn.Module):
    def __init__(self, mu_x, x_mask):
        super().__init__()
        self.mu_x, self.x_mask = mu_x, x_mask

    def forward(self, x, c, x_lengths):
        return torch.zeros(self.mu_x.shape[0], 4, self.mu_x.shape[2], dtype=self.mu_x.dtype), self.mu_x, self.x_mask


class _Dp(torch.nn.Module):
    def __init__(self, logw):
        super().__init__()
        self.logw = logw

    def forward(self, x, x_mask, c):
        return self.logw


class _RefEncoder(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.dtype = dtype

    def forward(self, z, z_mask):
        return torch.ones(z.shape[0], GIN, dtype=self.dtype)


class _Decoder(torch.nn.Module):
    def __init__(self, W):
        super().__init__()
        self.W, self.seen = W, {}

    def compute_loss(self, x1, mask, mu, c):
        self.seen = dict(mu=mu.detach().clone(), c=c.detach().clone())
        return torch.sum(self.W * mu), None


def run_forward(StableTTS, case, dtype, cfg_dropout, seed):
    """The reference forward on the case's inputs in `dtype`; -> losses, gradients, attn, the mask drawn, mu_y_masked."""
    B, M, Tx = case["mu_x"].shape
    Ty = case["y"].shape[2]
    model = StableTTS(10, M, 16, 16, 2, 1, 2, 3, 0.0, GIN).to(dtype)
    mu_x = torch.from_numpy(case["mu_x"]).to(dtype).requires_grad_(True)
    logw = torch.from_numpy(case["logw"]).to(dtype).requires_grad_(True)
    x_lengths, y_lengths = torch.from_numpy(case["x_lengths"]), torch.from_numpy(case["y_lengths"])
    x_mask = (torch.arange(Tx)[None] < x_lengths[:, None]).unsqueeze(1).to(dtype)
    model.encoder, model.dp, model.ref_encoder = _Encoder(mu_x, x_mask), _Dp(logw), _RefEncoder(dtype)
    model.decoder = _Decoder(torch.from_numpy(case["W"]).to(dtype))
    with torch.no_grad():
        model.fake_content.copy_(torch.from_numpy(case["fake_content"]).to(dtype))     # fake_speaker stays 0: c shows the mask
    model.cfg_dropout = cfg_dropout
    y = torch.from_numpy(case["y"]).to(dtype)
    torch.manual_seed(seed)
    dur_loss, diff_loss, prior_loss, attn = model(torch.zeros(B, Tx, dtype=torch.long), x_lengths, y, y_lengths, y[:, :, :4],
                                                  torch.full((B,), 4))
    (dur_loss + diff_loss + prior_loss).backward()
    keep = (model.decoder.seen["c"][:, 0] == 1)
    return dict(dur_loss=dur_loss.detach(), diff_loss=diff_loss.detach(), prior_loss=prior_loss.detach(), attn=attn.detach(),
                keep=keep, mu_y_masked=model.decoder.seen["mu"], grad_mu_x=mu_x.grad, grad_logw=logw.grad,
                grad_fake_content=model.fake_content.grad)


def with_sum(rng, d, total):
    """d (every entry >= 1) nudged entry by entry until it sums to total."""
    d = np.array(d, np.int64)
    while d.sum() != total:
        i = rng.integers(0, len(d))
        d[i] += 1 if d.sum() < total else (-1 if d[i] > 1 else 0)
    return d


def make_inputs(rng, M, Tx, Ty, durs):
    """durs: per item the ground-truth frames per token (its length is t_x, its sum t_y)."""
    B = len(durs)
    x_lengths = np.array([len(d) for d in durs], np.int64)
    y_lengths = np.array([int(np.sum(d)) for d in durs], np.int64)
    assert x_lengths.max() == Tx and y_lengths.max() == Ty
    mu_x = rng.standard_normal((B, M, Tx)).astype(np.float32)
    noise = (np.clip(np.rint(rng.standard_normal((B, M, Ty)) * 0.3 * 64), -127, 127) / 64).astype(np.float32)
    y = np.zeros((B, M, Ty), np.float32)
    logw = np.zeros((B, 1, Tx), np.float32)
    for b, d in enumerate(durs):
        idx = np.repeat(np.arange(len(d)), d)
        y[b, :, :len(idx)] = mu_x[b][:, idx] + noise[b, :, :len(idx)]
        logw[b, 0, :len(d)] = np.log(np.maximum(np.asarray(d, np.float32), 0.5)) + 0.2 * rng.standard_normal(len(d)).astype(np.float32)
    W = (rng.integers(-8, 9, size=(B, M, Ty)) / 4).astype(np.float32)
    fake_content = rng.standard_normal((1, M, 1)).astype(np.float32)
    return dict(x_lengths=x_lengths, y_lengths=y_lengths, mu_x=mu_x, logw=logw, y=y, W=W, fake_content=fake_content)


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE")
    if not ref_dir or not os.path.isdir(os.path.join(ref_dir, "models")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, ref_dir)
    torch.set_num_threads(1)
    _install_standins()
    StableTTS = importlib.import_module("models.model").StableTTS          # reference, unmodified
    import monotonic_align
    assert os.path.dirname(monotonic_align.__file__) == os.path.join(os.path.abspath(ref_dir), "monotonic_align")
    from tests import align_loss_restatement as ar
    from tools.make_golden_mas import masks, neg_cent_of
    rng = np.random.default_rng(20261018)
    out = {}

    def add(name, case, cfg_dropout, seed, want_mixed):
        r32 = run_forward(StableTTS, case, torch.float32, cfg_dropout, seed)
        r64 = run_forward(StableTTS, case, torch.float64, cfg_dropout, seed)
        allk = run_forward(StableTTS, case, torch.float32, -1.0, seed)        # every item kept: mu_y_masked is mu_y
        keep = r32["keep"]
        assert torch.equal(keep, r64["keep"]) and torch.equal(r32["attn"], r64["attn"].float()) and allk["keep"].all()
        assert torch.equal(r32["attn"], allk["attn"])
        if want_mixed:
            assert keep.any() and not keep.all(), keep
        attn = r32["attn"]                                                  # (B, Tx, Ty)
        x_mask, y_mask, attn_mask = masks(case["x_lengths"].tolist(), case["y_lengths"].tolist(), attn.shape[1], attn.shape[2])
        nc = neg_cent_of(torch.from_numpy(case["mu_x"]), torch.from_numpy(case["y"]))
        for trial in range(4):
            sign = torch.from_numpy(rng.choice([-1.0, 1.0], size=nc.shape).astype(np.float32))
            again = monotonic_align.maximum_path(nc * (1 + 1e-5 * sign), attn_mask)
            assert torch.equal(again.transpose(1, 2), attn), f"{name}: the path moves under 1e-5 perturbations (trial {trial})"
        durations = attn.sum(2).to(torch.int32).numpy()
        # the restatement agrees with the float64 run before anything is written
        c64 = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in case.items()}
        f = ar.forward(c64["mu_x"], x_mask.numpy(), c64["logw"], case["x_lengths"], c64["y"], y_mask.numpy(), durations,
                       keep.numpy(), c64["fake_content"])
        assert abs(f["prior_loss"] - float(r64["prior_loss"])) <= 1e-12 * abs(f["prior_loss"])
        assert abs(f["dur_loss"] - float(r64["dur_loss"])) <= 1e-12 * abs(f["dur_loss"])
        assert np.array_equal(f["mu_y"].astype(np.float32), allk["mu_y_masked"].numpy())
        for k, v in case.items():
            out[f"{name}/{k}"] = v
        out[f"{name}/keep"] = keep.numpy()
        out[f"{name}/durations"] = durations
        out[f"{name}/attn"] = attn.numpy().astype(np.uint8)
        out[f"{name}/mu_y"] = allk["mu_y_masked"].numpy()
        out[f"{name}/mu_y_masked"] = r32["mu_y_masked"].numpy()
        for k in ("dur_loss", "diff_loss", "prior_loss", "grad_mu_x", "grad_logw", "grad_fake_content"):
            out[f"{name}/{k}"] = r32[k].numpy()
            out[f"{name}/{k}_f64"] = r64[k].numpy()
        print(f"{name}: keep {keep.tolist()}, t_x {case['x_lengths'].tolist()}, t_y {case['y_lengths'].tolist()}, "
              f"longest token {int(durations.max())}, tokens of 1 frame {int((durations == 1).sum())}, "
              f"tokens of 0 frames inside t_x {int(sum((durations[b, :n] == 0).sum() for b, n in enumerate(case['x_lengths'])))}")

    # ragged: item 0 at full length in both; item 1 holds the token of 270 frames and 19 tokens sharing 30 frames
    d0 = with_sum(rng, rng.integers(1, 16, size=37), 300)
    d1 = np.ones(20, np.int64)
    d1[7] = 270
    d1[[2, 3, 11, 12, 13, 16]] = [3, 2, 2, 3, 2, 5]
    assert d1.sum() == 300 and (d1 == 1).sum() >= 10
    d2 = rng.integers(1, 9, size=29)
    d3 = rng.integers(1, 10, size=12)
    ragged = make_inputs(rng, 80, 37, 300, [d0, d1, d2, d3])
    seed = next(s for s in range(100) if 0 < int((torch.manual_seed(s) and torch.rand(4, 1) > 0.2).sum()) < 4)
    add("ragged", ragged, 0.2, seed, True)

    # wide: item 0 has 30 tokens and 18 frames: the search gives the first 12 tokens no frame
    w0 = np.array([0] * 12 + [1] * 18)
    wide = make_inputs(rng, 100, 30, 40, [w0, with_sum(rng, rng.integers(1, 5, size=14), 40), rng.integers(1, 4, size=9)])
    seed = next(s for s in range(100) if 0 < int((torch.manual_seed(s) and torch.rand(3, 1) > 0.2).sum()) < 3)
    add("wide", wide, 0.2, seed, True)

    # edges: t_x = 1; t_y = 1 with t_x = 5; every token and frame valid
    e2 = with_sum(rng, rng.integers(1, 6, size=12), 40)
    edges = make_inputs(rng, 80, 12, 40, [np.array([33]), np.array([0, 0, 0, 0, 1]), e2])
    add("edges_dropped", edges, 2.0, 0, False)
    add("edges_kept", edges, -1.0, 0, False)

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    _save(OUT, out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} kB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
