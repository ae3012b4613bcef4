"""Checks of a native CFM decoder against the fp32 oracle, shared by the GPU tests that sweep the decoder's dimensions
(test_gpu_channel_widths.py: mel channels; test_gpu_decoder_configs.py: filter channels, gin channels, depth).

Gates are the ones of test_gpu_parity.py (evaluation, solve) and test_gpu_training.py (loss, gradients), raised to 1.5x the
operand-rounding floor where that is higher: the error of the fp32 oracle itself when only its weight matrices are rounded to
the operand type.  Every check prints its measured error next to its gate.
"""
import math

import numpy as np
import torch

import oracle

NFE_TOL = {"bf16": 1e-2, "f16": 7e-4}      # test_gpu_parity.py
MEL_TOL = 1e-3
DISP_TOL = {"bf16": 1e-2, "f16": 7e-4}
TOL = {"f16": 3e-3, "bf16": 2e-2}          # test_gpu_training.py: parameter gradients except the q / k projections, d mu, d c
TOL_QK = {"f16": 1e-2, "bf16": 1e-1}       # test_gpu_training.py: the q / k projections (conditioning of d q, d k at random init)
TOL_QK_SIZE = {"f16": 8e-2, "bf16": 3e-1}  # test_gpu_training.py: its q / k gates at size (end to end, with a cosine)
COS_QK_SIZE = {"f16": 0.999, "bf16": 0.97}
TOL_QK_MATCHED = {"f16": 1e-2, "bf16": 6e-2}   # test_gpu_training.py: q / k against the oracle evaluated at the native q, k, v
LOSS_TOL = {"f16": 5e-4, "bf16": 3e-3}

B, T, LENGTHS = 3, 130, [130, 97, 41]      # ragged; 130 frames span three 64-frame tiles and one partial 32-frame chunk
GUARD = 1 << 18                            # tail guard of the caller-owned gradient buffer: 1 MB of floats
SENTINEL = 0x7FBADBAD                      # a NaN bit pattern no kernel produces


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cos(a, b):
    """Cosine in fp64 without a floor on the norms (these gradients are ~1e-6: torch's eps = 1e-8 on the product would swallow them)."""
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float(a @ b / max(float(a.norm() * b.norm()), 1e-300))


def is_qk(name):
    return ".attn.conv_q." in name or ".attn.conv_k." in name


def round_weights(sd, dt):
    """The state dict with every weight matrix rounded to the operand type (biases and norms stay fp32)."""
    r = torch.float16 if dt == "f16" else torch.bfloat16
    return {k: (v.to(r).float() if v.dim() > 1 else v) for k, v in sd.items()}


def check_evaluation_and_solve(label, dec, sd, inp, fs, fc, dt):
    """One evaluation at t = 0.4 and a 3-step Euler CFG solve against oracle.decoder_forward / cfm_forward.  Padded frames of the
    evaluation are exactly zero, those of the solve exactly z."""
    t = torch.tensor(0.4)
    ref1 = oracle.decoder_forward(sd, t, inp["z"], inp["mask"], inp["mu"], inp["c"])
    one = dec.estimator(t.cuda(), inp["z"].cuda(), inp["mask"].cuda(), inp["mu"].cuda(), inp["c"].cuda()).cpu()
    pad = ~inp["mask"].bool().expand_as(one)
    assert one.shape == ref1.shape and torch.isfinite(one).all()
    assert float(one[pad].abs().max()) == 0.0
    ref = oracle.cfm_forward(sd, inp["mu"], inp["mask"], 3, inp["z"], inp["c"], "euler",
                             dict(fake_speaker=fs, fake_content=fc, cfg_strength=3.0))
    kw = dict(fake_speaker=fs.cuda(), fake_content=fc.cuda(), cfg_strength=3.0)
    out = dec(inp["mu"].cuda(), inp["mask"].cuda(), 3, 1.0, inp["c"].cuda(), "euler", kw, z=inp["z"].cuda()).cpu()
    assert torch.isfinite(out).all() and torch.equal(out[pad], inp["z"][pad])
    floor = rel(oracle.decoder_forward(round_weights(sd, dt), t, inp["z"], inp["mask"], inp["mu"], inp["c"]), ref1)
    gate1 = max(NFE_TOL[dt], 1.5 * floor)
    e1, mel = rel(one, ref1), rel(out, ref)
    disp = float((out.double() - ref.double()).abs().max() / (ref.double() - inp["z"].double()).abs().max())
    print(f"[{label} {dt}] one evaluation {e1:.2e} (gate {gate1:.1e}, rounding floor {floor:.1e}); 3-step Euler CFG solve: mel {mel:.2e} "
          f"(gate {MEL_TOL:.0e}), displacement {disp:.2e} (gate {DISP_TOL[dt]:.0e})")
    assert e1 <= gate1 and mel <= MEL_TOL and disp <= DISP_TOL[dt], (e1, mel, disp)


def native_qkv(eng, b, t, n_layers, h=4):
    """The training forward's attention operands of every block as the kernels saw them (debug capture on), as oracle.attention's
    qkv_subst: post-RoPE q without its log2(e) / sqrt(64) pre-scale, k, and v from its 16-bit plane plus its rounding residuals."""
    tp = (t + 63) // 64 * 64
    tt = np.arange(tp)
    pos = (tt & ~12) | ((tt & 4) << 1) | ((tt & 8) >> 1)      # v's frame order inside 16-frame groups
    out = []
    for i in range(n_layers):
        q = eng.debug_fetch(f"t{i}.q").reshape(b, h, t, 64) * (8.0 / math.log2(math.e))
        k = eng.debug_fetch(f"t{i}.k").reshape(b, h, t, 64)
        v = eng.debug_fetch(f"t{i}.vt").reshape(b, h, 64, tp).astype(np.float64)
        try:
            v = v + eng.debug_fetch(f"t{i}.vtlo").reshape(b, h, 64, tp).astype(np.float64)
        except Exception:      # noqa: BLE001  (ST_TRAIN_VLO=0: no residual plane)
            pass
        v = v[..., pos][..., :t].transpose(0, 1, 3, 2).astype(np.float32)
        out.append({nm: torch.from_numpy(np.ascontiguousarray(a)) for nm, a in (("q", q), ("k", k), ("v", v))})
    return out


def check_qk_matched(label, subst, params, sd, x1, inp, t_rand, z, dt):
    """The q / k projections' gradients against the oracle's autograd evaluated AT the native forward's own q, k, v (straight-through,
    oracle.attention(subst=...)).  That removes the amplification of the forward's operand rounding by the conditioning of d q, d k
    and leaves the native backward chain compared end to end; gate test_gpu_training.py's TOL_QK_MATCHED."""
    with torch.enable_grad():
        pm = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        oracle.compute_loss(pm, x1, inp["mask"], inp["mu"], inp["c"], t_rand, z, qkv_subst=subst)[0].backward()
    wm = {n: rel(params[n].grad.cpu(), pm[n].grad) for n in params if is_qk(n)}
    cm = min(cos(params[n].grad.cpu(), pm[n].grad) for n in params if is_qk(n))
    worst = max((v, k) for k, v in wm.items())
    print(f"[{label} {dt}] q/k gradients vs the oracle at the native q, k, v: worst {worst[0]:.2e} ({worst[1]}, gate "
          f"{TOL_QK_MATCHED[dt]:.0e}), min cosine {cm:.6f}")
    assert worst[0] <= TOL_QK_MATCHED[dt], wm
    return worst[0]


def check_loss_and_gradients(label, dec, sd, inp, x1, t_rand, z, dt, qk_at_size=False):
    """The loss, every parameter gradient, d mu and d c of the native compute_loss + backward against the oracle's autograd.  The
    set of gradient names must equal the reference's.  The q / k projections are also held to a cosine, and to the oracle evaluated
    at the native q, k, v (check_qk_matched).  qk_at_size: hold them end to end to the at-size gate instead of TOL_QK."""
    eng = dec.estimator.engine()
    mu = inp["mu"].cuda().requires_grad_(True)
    c = inp["c"].cuda().requires_grad_(True)
    eng.debug_capture(True)
    try:
        loss, _ = dec.compute_loss(x1.cuda(), inp["mask"].cuda(), mu, c, t_rand=t_rand.cuda(), z=z.cuda())
        loss.backward()
        n_layers = sum(1 for k in sd if k.endswith(".time_fusion.film.weight"))
        subst = native_qkv(eng, x1.shape[0], x1.shape[2], n_layers)
    finally:
        eng.debug_capture(False)
    pr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    mur, cr = inp["mu"].clone().requires_grad_(True), inp["c"].clone().requires_grad_(True)
    lref, _ = oracle.compute_loss(pr, x1, inp["mask"], mur, cr, t_rand, z)
    lref.backward()
    pf = {k: v.clone().requires_grad_(True) for k, v in round_weights(sd, dt).items()}
    oracle.compute_loss(pf, x1, inp["mask"], inp["mu"], inp["c"], t_rand, z)[0].backward()
    gate = {n: max(TOL[dt], 1.5 * rel(pf[n].grad, pr[n].grad)) for n in pr}
    el = abs(float(loss.detach()) - float(lref.detach())) / float(lref.detach())
    params = dict(dec.estimator.named_parameters())
    assert set(params) == set(pr)
    for n, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    worst = {n: rel(params[n].grad.cpu(), pr[n].grad) for n in params}
    emu, ec = rel(mu.grad.cpu(), mur.grad), rel(c.grad.cpu(), cr.grad)
    cs = {n: cos(params[n].grad.cpu(), pr[n].grad) for n in params if is_qk(n)}
    nq = max((v / gate[k], v, k) for k, v in worst.items() if not is_qk(k))
    wq = max(v for k, v in worst.items() if is_qk(k))
    qk_gate = TOL_QK_SIZE[dt] if qk_at_size else TOL_QK[dt]
    print(f"[{label} {dt}] loss {el:.2e} (gate {LOSS_TOL[dt]:.0e}); non-q/k gradients: closest to its gate {nq[1]:.2e} ({nq[2]}, gate "
          f"{gate[nq[2]]:.1e}), worst {max(v for k, v in worst.items() if not is_qk(k)):.2e}; q/k {wq:.2e} (gate {qk_gate:.0e}, cosine "
          f"{min(cs.values()):.6f}, gate {COS_QK_SIZE[dt]}); d mu {emu:.2e}, d c {ec:.2e} (gate {TOL[dt]:.0e})")
    check_qk_matched(label, subst, params, sd, x1, inp, t_rand, z, dt)
    assert el <= LOSS_TOL[dt]
    bad = {k: v for k, v in worst.items() if v > (qk_gate if is_qk(k) else gate[k])}
    assert not bad, bad
    assert min(cs.values()) >= COS_QK_SIZE[dt], cs
    assert emu <= TOL[dt] and ec <= TOL[dt], (emu, ec)


def _backward_into_own_buffer(dec, t, inp, g, check=None):
    """Native forward + the three backward parts through the engine binding, every parameter gradient written into a caller-owned
    flat buffer of st_train_grad_numel() floats followed by a tail guard; the whole allocation starts as SENTINEL.  check(part, buffer)
    runs after each part (the device synchronised)."""
    eng = dec.estimator.engine()
    stream = torch.cuda.current_stream().cuda_stream
    n = eng.grad_layout()[None]
    big = torch.empty(n + GUARD, device="cuda", dtype=torch.float32)
    big.view(torch.int32).fill_(SENTINEL)
    x, mu, mask, c = (inp[k].cuda().contiguous() for k in ("z", "mu", "mask", "c"))
    out = torch.empty_like(x)
    eng.train_forward(t, x, mu, mask, c, out, 0.0, 0, stream)
    serial = eng.train_serial()
    gx, gmu, gc = torch.empty_like(x), torch.empty_like(mu), torch.empty_like(c)
    for part, args in ((0, (g, big[:n], None, None, None)), (1, (None, None, None, None, None)), (2, (None, None, gx, gmu, gc))):
        eng.train_backward_part(serial, part, x.shape[0], x.shape[2], *args, stream)
        torch.cuda.synchronize()
        if check is not None:
            check(part, big.cpu())
    return big.cpu(), out.cpu(), gx.cpu(), gmu.cpu(), gc.cpu()


def check_backward_bounds(label, make_decoder, inp, t, g, monkeypatch):
    """The backward runs in three parts (st_train_backward_part), each writing the gradients of its own parameters.  After part p,
    every float of a caller-owned gradient buffer outside the slices of the parameters of parts 0..p -- the slices of later parts, the
    64-byte alignment gaps and a 1 MB tail guard -- still holds the sentinel.  At the end each slice equals the gradient the autograd
    path produced, and the single-stream order (ST_TRAIN_SIDE=0) gives the same buffer bit for bit.  make_decoder() returns a fresh
    f16 decoder."""
    dec = make_decoder()
    x = inp["z"].cuda().requires_grad_(True)
    mu = inp["mu"].cuda().requires_grad_(True)
    c = inp["c"].cuda().requires_grad_(True)
    out_ag = dec.estimator(t, x, inp["mask"].cuda(), mu, c)
    out_ag.backward(g)
    want = {n: p.grad.cpu().clone() for n, p in dec.estimator.named_parameters()}
    want_in = (out_ag.detach().cpu(), x.grad.cpu(), mu.grad.cpu(), c.grad.cpu())

    eng = dec.estimator.engine()
    lay = eng.grad_layout()
    n = lay[None]
    slices = {name: v for name, v in lay.items() if name is not None}
    assert set(slices) == set(want)
    written = [torch.zeros(n + GUARD, dtype=torch.bool) for _ in range(3)]      # slices of parts 0..p
    for name, (off, k, _) in slices.items():
        assert off + k <= n, name
        for p in range(eng.param_part(name), 3):
            written[p][off:off + k] = True
    assert not written[2][n:].any()

    def check(part, buf):
        stray = ((~written[part]) & (buf.view(torch.int32) != SENTINEL)).nonzero().flatten()
        where = sorted({nm for nm, (off, k, _) in slices.items() if stray.numel() and ((stray >= off) & (stray < off + k)).any()})
        print(f"[{label}] after backward part {part}: {stray.numel()} floats written outside the slices of parts 0..{part}"
              + (f" ({int(stray[0])}..{int(stray[-1])}; inside {where})" if stray.numel() else ""))
        assert stray.numel() == 0, (part, where)

    monkeypatch.delenv("ST_TRAIN_SIDE", raising=False)
    res = _backward_into_own_buffer(dec, t, inp, g, check)
    big = res[0]
    print(f"[{label}] flat gradient buffer: {n} floats, {int((~written[2][:n]).sum())} of them gaps, {GUARD} guard")
    for name, (off, k, shape) in slices.items():
        assert torch.equal(big[off:off + k].view(shape), want[name]), name
    for a, b in zip(res[1:], want_in):
        assert torch.equal(a, b)

    monkeypatch.setenv("ST_TRAIN_SIDE", "0")          # read when the engine first trains: a fresh decoder
    res1 = _backward_into_own_buffer(make_decoder(), t, inp, g, check)
    assert torch.equal(res1[0].view(torch.int32), big.view(torch.int32))
    for a, b in zip(res1[1:], res[1:]):
        assert torch.equal(a, b)
