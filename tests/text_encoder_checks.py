"""Checks of a native TextEncoder against the oracle (oracle.text_encoder_forward, fp64 on the CPU), shared by the GPU tests of
its training path (test_gpu_text_encoder_training.py) and the sweep of its dimensions (test_gpu_text_encoder_configs.py).

Gates are the ones of test_gpu_text_encoder.py (forward) and test_gpu_training.py (loss, gradients), raised to 1.5x the
operand-rounding floor where that is higher: the error of the oracle itself when only its weight matrices are rounded to the
operand type (decoder_checks.round_weights).  The floor comes from the oracle alone.  Every check prints its measured error next
to its gate.
"""
import numpy as np
import torch

import oracle
from decoder_checks import B, GUARD, LENGTHS, SENTINEL, T, TOL, TOL_QK, cos, is_qk, rel, round_weights      # noqa: F401

TOL_X = {"bf16": 3e-3, "f16": 3e-4}        # test_gpu_text_encoder.py: x, the fp32 residual stream fed by 16-bit-operand GEMMs
TOL_MU = {"bf16": 2e-3, "f16": 3e-4}       # test_gpu_text_encoder.py: mu_x, one more 16-bit-operand GEMM on top


def loss_weights(B, T, seed, out_channels=128, hidden=256):      # = tools/make_golden_text_encoder_grads.py: loss_weights
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    w_mu = rng.standard_normal((B, out_channels, T)).astype(np.float32)
    w_x = (rng.standard_normal((B, hidden, T)) * 0.1).astype(np.float32)
    return torch.from_numpy(w_mu), torch.from_numpy(w_x)


def _loss(x, mu_x, w_mu, w_x):
    """(mu_x * w_mu).sum() + (x * w_x).sum(); a weight that is None leaves its term out (a loss from one output only)."""
    terms = [(o * w.to(device=o.device, dtype=o.dtype)).sum() for o, w in ((mu_x, w_mu), (x, w_x)) if w is not None]
    return terms[0] + terms[1] if len(terms) == 2 else terms[0]


def oracle_grads(sd, tok, c, lens, w_mu, w_x, fwd=None):
    """loss, d c and every parameter gradient of fp64 autograd through the oracle (fwd(params, c) -> x, mu_x: another forward on
    the same parameters).  A parameter the loss does not reach has gradient None."""
    with torch.enable_grad():
        pr = {k: v.clone().double().requires_grad_(True) for k, v in sd.items()}
        cc = c.clone().double().requires_grad_(True)
        if fwd is None:
            x, mu_x, _ = oracle.text_encoder_forward(pr, tok, cc, lens)
        else:
            x, mu_x = fwd(pr, cc)
        loss = _loss(x, mu_x, w_mu, w_x)
        loss.backward()
    return float(loss.detach()), cc.grad, {n: p.grad for n, p in pr.items()}


def n_layers_of(sd):
    return sum(1 for k in sd if k.endswith(".attn.conv_q.weight"))


def reference(sd, tok, c, lens, w_mu, w_x):
    """The fp64 oracle on one case: the forward's x, mu_x, mask and oracle_grads' loss, d c, gradients."""
    with torch.no_grad():
        x, mu_x, mask = oracle.text_encoder_forward({k: v.double() for k, v in sd.items()}, tok, c.double(), lens)
    loss, gc, grads = oracle_grads(sd, tok, c, lens, w_mu, w_x)
    return dict(x=x, mu_x=mu_x, mask=mask.float(), loss=loss, gc=gc, grads=grads)


def rounding_floor(ref, sd, tok, c, lens, w_mu, w_x, dt):
    """The oracle's own error against `ref` when only its weight matrices are rounded to the operand type: of x, mu_x and of every
    gradient (None where the loss does not reach the parameter)."""
    rf = reference(round_weights(sd, dt), tok, c, lens, w_mu, w_x)
    return dict(x=rel(rf["x"], ref["x"]), mu_x=rel(rf["mu_x"], ref["mu_x"]),
                grads={n: (rel(rf["grads"][n], g) if g is not None else None) for n, g in ref["grads"].items()})


def module(cfg, sd, dt, train=False):
    from stabletts_amd.text_encoder import TextEncoder
    m = TextEncoder(cfg.n_vocab, cfg.out_channels, cfg.hidden_channels, cfg.filter_channels, cfg.n_heads, cfg.n_layers, cfg.kernel_size,
                    cfg.p_dropout, cfg.gin_channels, operand_dtype=dt)
    m.load_state_dict(sd)
    m = m.cuda()
    return m.train() if train else m.eval()


def native_grads(m, tok, c, lens, w_mu, w_x, c_grad=True):
    """loss, d c (None without c_grad) and the .grad of every parameter of the native module (None where autograd left none)."""
    m.zero_grad(set_to_none=True)
    cc = c.cuda().clone().requires_grad_(c_grad)
    with torch.enable_grad():
        x, mu_x, mask = m(tok.cuda(), cc, lens.cuda())
        assert not mask.requires_grad
        loss = _loss(x, mu_x, w_mu, w_x)
        loss.backward()
    return (float(loss.detach()), cc.grad.cpu() if c_grad else None,
            {n: (p.grad.detach().cpu().clone() if p.grad is not None else None) for n, p in m.named_parameters()})


def check_forward(label, m, tok, c, lens, ref, floor, dt):
    """The inference forward (no_grad) against the oracle: the mask equal, padded frames of x and mu_x exactly 0, x and mu_x within
    TOL_X / TOL_MU (or 1.5x the rounding floor)."""
    with torch.no_grad():
        x, mu_x, mask = (v.cpu() for v in m(tok.cuda(), c.cuda(), lens.cuda()))
    assert x.shape == ref["x"].shape and mu_x.shape == ref["mu_x"].shape
    assert torch.equal(mask, ref["mask"])
    assert torch.isfinite(x).all() and torch.isfinite(mu_x).all()
    assert float(x[~mask.bool().expand_as(x)].abs().max()) == 0.0
    assert float(mu_x[~mask.bool().expand_as(mu_x)].abs().max()) == 0.0
    gx, gmu = max(TOL_X[dt], 1.5 * floor["x"]), max(TOL_MU[dt], 1.5 * floor["mu_x"])
    ex, em = rel(x, ref["x"]), rel(mu_x, ref["mu_x"])
    print(f"[{label} {dt}] forward: x {ex:.2e} (gate {gx:.1e}, rounding floor {floor['x']:.1e}), mu_x {em:.2e} (gate {gmu:.1e}, rounding "
          f"floor {floor['mu_x']:.1e})")
    assert ex <= gx and em <= gmu, (ex, em)


def check_gradients(label, got, ref, floor, dt):
    """native_grads' result against the oracle's: the loss and d c within TOL, every gradient the oracle has within TOL (or 1.5x its
    rounding floor), the q / k projections within TOL_QK.  The set of names equals the oracle's."""
    lg, gcg, gg = got
    lr, gcr, gr = ref["loss"], ref["gc"], ref["grads"]
    assert set(gg) == set(gr)
    names = [n for n in gr if gr[n] is not None]
    for n in names:
        assert gg[n] is not None and gg[n].shape == gr[n].shape and torch.isfinite(gg[n]).all(), n
    gate = {n: TOL_QK[dt] if is_qk(n) else max(TOL[dt], 1.5 * floor["grads"][n]) for n in names}
    err = {n: rel(gg[n], gr[n]) for n in names}
    el = abs(lg - lr) / max(abs(lr), 1.0)
    ec = rel(gcg, gcr)
    nq = max((err[n] / gate[n], err[n], n) for n in names if not is_qk(n))
    wo = max(err[n] for n in names if not is_qk(n))
    wq = max((err[n], n) for n in names if is_qk(n))
    cs = min(cos(gg[n], gr[n]) for n in names if is_qk(n))
    print(f"[{label} {dt}] loss {el:.2e}, d c {ec:.2e} (gate {TOL[dt]:.0e}); non-q/k gradients: closest to its gate {nq[1]:.2e} ({nq[2]}, gate "
          f"{gate[nq[2]]:.1e}), worst {wo:.2e}; q/k {wq[0]:.2e} ({wq[1]}, gate {TOL_QK[dt]:.0e}), min cosine {cs:.6f}")
    assert el <= TOL[dt]
    assert ec <= TOL[dt]
    bad = {n: (v, gate[n]) for n, v in err.items() if v > gate[n]}
    assert not bad, bad


def embedding_gradient_reference(sd, tok, c, lens, w_mu, w_x):
    """d emb.weight = sqrt(C) * index_add over the valid rows, at the clamped ids, of the oracle's d x0 (x0: block 0's input)."""
    F = torch.nn.functional
    V, C = sd["emb.weight"].shape
    pr = {k: v.double() for k, v in sd.items()}
    ids = tok.clamp(0, V - 1)
    Tn = tok.shape[1]
    with torch.enable_grad():
        x0 = (F.embedding(ids, pr["emb.weight"]) * C ** 0.5).transpose(1, 2).detach().requires_grad_(True)
        mask = (torch.arange(Tn)[None] < lens[:, None]).unsqueeze(1).double()
        x = x0
        for i in range(n_layers_of(sd)):
            x = oracle.dit_conv_block(pr, f"encoder.{i}.", x, c.double(), mask)
        mu_x = F.conv1d(x, pr["proj.weight"], pr["proj.bias"]) * mask
        _loss(x, mu_x, w_mu, w_x).backward()
    dx0 = x0.grad.transpose(1, 2) * mask.transpose(1, 2)           # (B, T, C), valid rows only
    ref = torch.zeros(V, C, dtype=torch.float64).index_add_(0, ids.reshape(-1), dx0.reshape(-1, C)) * C ** 0.5
    used = torch.zeros(V, dtype=torch.bool)
    for b, n in enumerate(lens.tolist()):
        used[ids[b, :n]] = True
    return ref, used


def _direct(m, tok, c, lens, gx, gmu):
    """Native training forward + backward through the engine binding, every parameter gradient written into a caller-owned flat
    buffer of grad_layout()[None] floats followed by a tail guard; the whole allocation starts as SENTINEL."""
    eng = m.engine()
    stream = torch.cuda.current_stream().cuda_stream
    n = eng.grad_layout()[None]
    big = torch.empty(n + GUARD, device="cuda", dtype=torch.float32)
    big.view(torch.int32).fill_(SENTINEL)
    Bn, Tn = tok.shape
    tk, ln, cc = tok.cuda().contiguous(), lens.cuda().contiguous(), c.cuda().contiguous()
    f32 = dict(device="cuda", dtype=torch.float32)
    x = torch.empty(Bn, m.hidden_channels, Tn, **f32)
    mu_x = torch.empty(Bn, m.out_channels, Tn, **f32)
    mask = torch.empty(Bn, 1, Tn, **f32)
    eng.text_encoder_train_forward(tk, ln, cc, x, mu_x, mask, 0.0, 0, stream)
    gc = torch.empty_like(cc)
    eng.text_encoder_train_backward(eng.train_serial(), Bn, Tn, gx.cuda().contiguous(), gmu.cuda().contiguous(), big[:n], gc, stream)
    torch.cuda.synchronize()
    return big.cpu(), gc.cpu(), x.cpu(), mu_x.cpu()


def check_backward_bounds(label, make_module, tok, c, lens, w_mu, w_x, monkeypatch):
    """st_text_encoder_train_backward into a caller-owned gradient buffer: every float outside the parameter slices -- the 64-byte
    alignment gaps and a 1 MB tail guard -- still holds the sentinel, each slice equals the gradient the autograd path produced on
    the same inputs, and the single-stream order (ST_TRAIN_SIDE=0) gives the same buffer, d c, x and mu_x bit for bit.
    make_module() returns a fresh f16 module."""
    monkeypatch.delenv("ST_TRAIN_SIDE", raising=False)
    m = make_module()
    _, want_c, want = native_grads(m, tok, c, lens, w_mu, w_x)      # d loss / d mu_x = w_mu, d loss / d x = w_x
    lay = m.engine().grad_layout()
    n = lay[None]
    slices = {name: v for name, v in lay.items() if name is not None}
    assert set(slices) == set(want)
    written = torch.zeros(n + GUARD, dtype=torch.bool)
    for name, (off, k, _) in slices.items():
        assert off % 16 == 0 and off + k <= n and not written[off:off + k].any(), name
        written[off:off + k] = True

    def run(mod):
        big, gc, x, mu_x = _direct(mod, tok, c, lens, w_x, w_mu)
        stray = ((~written) & (big.view(torch.int32) != SENTINEL)).nonzero().flatten()
        print(f"[{label}] {n} floats, {int((~written[:n]).sum())} of them gaps, {GUARD} guard: {stray.numel()} floats written outside the slices"
              + (f" ({int(stray[0])}..{int(stray[-1])})" if stray.numel() else ""))
        assert stray.numel() == 0
        return big, gc, x, mu_x

    res = run(m)
    for name, (off, k, shape) in slices.items():
        assert torch.equal(res[0][off:off + k].view(shape), want[name]), name
    assert torch.equal(res[1], want_c)

    monkeypatch.setenv("ST_TRAIN_SIDE", "0")          # read when the engine first trains: a fresh module
    res1 = run(make_module())
    assert torch.equal(res1[0].view(torch.int32), res[0].view(torch.int32))
    for a, b in zip(res1[1:], res[1:]):
        assert torch.equal(a, b)
