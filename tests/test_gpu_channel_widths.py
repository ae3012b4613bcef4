"""Mel-channel counts other than 128 / 80 against the fp32 oracle on a real MI355X.  Run with ``-m gpu``.

The engine pads the mel channels to Mp = ceil(M / 128) * 128.  Every other test runs at M = 128 or 80 (Mp = 128); from Mp = 256 on
other code paths run: final_proj's weight gradient takes the TN GEMM + multi-output reduce (cout16 = Mp a multiple of 256, the last
64-column tile partial when M % 64 != 0), the fallback weight-gradient reduce with cout16 % 256 != 0 (Mp = 384), the two-source
in_proj operand and its weight gradient with c0 = Mp, cond_proj.0 over Mp input channels, the time-major transposes with M < Mp,
final_proj's dgrad and the inference final_proj with the CFG combine.

  M    Mp   why
  1    128  extreme padding; transposes with one real channel
  80   128  control (the existing baseline)
  200  256  TN weight gradient, partial last 64-column tile
  256  256  TN weight gradient, full tiles
  300  384  fallback weight-gradient reduce with cout16 % 256 != 0
  450  512  TN weight gradient, two 256 tiles, partial 64-column tile

Gates are the ones of test_gpu_parity.py (evaluation, solve) and test_gpu_training.py (loss, gradients), raised to 1.5x the
operand-rounding floor where that is higher: the error of the fp32 oracle itself when only its weight matrices are rounded to the
operand type.  At M >= 80 the floor stays below two thirds of every gate, so the gates printed are the modules' own.  At M = 1 it does
not: one output channel averages no rounding error away.  There the evaluation floor is 1.2e-3 (native 1.3e-3), and the floor of
final_proj.bias, a one-element gradient, is 6.3e-3 (native 4.3e-3).  The gradients of the q / k projections depend on the v and h1
operands, which that floor does not round.  So at M = 1 they are held to test_gpu_training.py's at-size gate and cosine instead
(measured 1.4e-2).  The bounds test checks that the backward writes nothing outside the parameter slices of a caller-owned flat
gradient buffer.
"""
import functools

import pytest
import torch

import oracle
from oracle.inputs import make_inputs

pytestmark = pytest.mark.gpu

WIDTHS = [1, 80, 200, 256, 300, 450]
CASES = [(m, "f16") for m in WIDTHS] + [(200, "bf16"), (300, "bf16")]

NFE_TOL = {"bf16": 1e-2, "f16": 7e-4}      # test_gpu_parity.py
MEL_TOL = 1e-3
DISP_TOL = {"bf16": 1e-2, "f16": 7e-4}
TOL = {"f16": 3e-3, "bf16": 2e-2}          # test_gpu_training.py: parameter gradients except the q / k projections, d mu, d c
TOL_QK = {"f16": 1e-2, "bf16": 1e-1}       # test_gpu_training.py: the q / k projections (conditioning of d q, d k at random init)
TOL_QK_SIZE, COS_QK_SIZE = 8e-2, 0.999     # test_gpu_training.py: its f16 q / k gates at size; here for M = 1 only
LOSS_TOL = {"f16": 5e-4, "bf16": 3e-3}

B, T, LENGTHS = 3, 130, [130, 97, 41]      # ragged; 130 frames span three 64-frame tiles and one partial 32-frame chunk
GUARD = 1 << 18                            # tail guard of the caller-owned gradient buffer: 1 MB of floats
SENTINEL = 0x7FBADBAD                      # a NaN bit pattern no kernel produces


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _cos(a, b):
    """Cosine in fp64 without a floor on the norms (these gradients are ~1e-6: torch's eps = 1e-8 on the product would swallow them)."""
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / max(float(a.norm() * b.norm()), 1e-300))


def _is_qk(name):
    return ".attn.conv_q." in name or ".attn.conv_k." in name


def _config(m):
    return oracle.DecoderConfig(noise_channels=m, cond_channels=m, out_channels=m)


@functools.lru_cache(maxsize=None)
def _state_dict(m):
    return oracle.make_state_dict(700 + m, _config(m))


def _round(sd, dt):
    """The state dict with every weight matrix rounded to the operand type (biases and norms stay fp32)."""
    r = torch.float16 if dt == "f16" else torch.bfloat16
    return {k: (v.to(r).float() if v.dim() > 1 else v) for k, v in sd.items()}


def _decoder(m, dt):
    from stabletts_amd.flow_matching import CFMDecoder
    d = CFMDecoder(m, m, 256, m, 1024, 4, 6, 3, 0.1, 256, operand_dtype=dt)
    d.estimator.load_state_dict(_state_dict(m))
    return d.cuda().eval()


@pytest.mark.parametrize("m,dt", CASES)
def test_evaluation_and_solve_vs_oracle(m, dt):
    sd = _state_dict(m)
    dec = _decoder(m, dt)
    inp = make_inputs(B, T, seed=m, lengths=LENGTHS, n_feats=m)
    t = torch.tensor(0.4)
    ref1 = oracle.decoder_forward(sd, t, inp["z"], inp["mask"], inp["mu"], inp["c"])
    one = dec.estimator(t.cuda(), inp["z"].cuda(), inp["mask"].cuda(), inp["mu"].cuda(), inp["c"].cuda()).cpu()
    pad = ~inp["mask"].bool().expand_as(one)
    assert one.shape == ref1.shape and torch.isfinite(one).all()
    assert float(one[pad].abs().max()) == 0.0
    fs, fc = oracle.make_cfg_params(4321 + m, _config(m))
    ref = oracle.cfm_forward(sd, inp["mu"], inp["mask"], 3, inp["z"], inp["c"], "euler",
                             dict(fake_speaker=fs, fake_content=fc, cfg_strength=3.0))
    kw = dict(fake_speaker=fs.cuda(), fake_content=fc.cuda(), cfg_strength=3.0)
    out = dec(inp["mu"].cuda(), inp["mask"].cuda(), 3, 1.0, inp["c"].cuda(), "euler", kw, z=inp["z"].cuda()).cpu()
    assert torch.isfinite(out).all() and torch.equal(out[pad], inp["z"][pad])
    floor = _rel(oracle.decoder_forward(_round(sd, dt), t, inp["z"], inp["mask"], inp["mu"], inp["c"]), ref1)
    gate1 = max(NFE_TOL[dt], 1.5 * floor)
    e1, mel = _rel(one, ref1), _rel(out, ref)
    disp = float((out.double() - ref.double()).abs().max() / (ref.double() - inp["z"].double()).abs().max())
    print(f"[M={m} {dt}] one evaluation {e1:.2e} (gate {gate1:.1e}, rounding floor {floor:.1e}); 3-step Euler CFG solve: mel {mel:.2e} (gate {MEL_TOL:.0e}), "
          f"displacement {disp:.2e} (gate {DISP_TOL[dt]:.0e})")
    assert e1 <= gate1 and mel <= MEL_TOL and disp <= DISP_TOL[dt], (e1, mel, disp)


@pytest.mark.grad
@pytest.mark.parametrize("m,dt", CASES)
def test_loss_and_every_gradient_vs_oracle_autograd(m, dt):
    sd = _state_dict(m)
    dec = _decoder(m, dt)
    inp = make_inputs(B, T, seed=100 + m, lengths=LENGTHS, n_feats=m)
    x1 = make_inputs(B, T, seed=200 + m, n_feats=m)["z"]
    g0 = torch.Generator().manual_seed(m)
    t_rand = torch.rand(B, 1, 1, generator=g0)
    z = torch.randn(B, m, T, generator=g0)
    mu = inp["mu"].cuda().requires_grad_(True)
    c = inp["c"].cuda().requires_grad_(True)
    loss, _ = dec.compute_loss(x1.cuda(), inp["mask"].cuda(), mu, c, t_rand=t_rand.cuda(), z=z.cuda())
    loss.backward()
    pr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    mur, cr = inp["mu"].clone().requires_grad_(True), inp["c"].clone().requires_grad_(True)
    lref, _ = oracle.compute_loss(pr, x1, inp["mask"], mur, cr, t_rand, z)
    lref.backward()
    pf = {k: v.clone().requires_grad_(True) for k, v in _round(sd, dt).items()}
    oracle.compute_loss(pf, x1, inp["mask"], inp["mu"], inp["c"], t_rand, z)[0].backward()
    gate = {n: max(TOL[dt], 1.5 * _rel(pf[n].grad, pr[n].grad)) for n in pr}
    el = abs(float(loss.detach()) - float(lref.detach())) / float(lref.detach())
    params = dict(dec.estimator.named_parameters())
    assert set(params) == set(pr)
    for n, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    worst = {n: _rel(params[n].grad.cpu(), pr[n].grad) for n in params}
    emu, ec = _rel(mu.grad.cpu(), mur.grad), _rel(c.grad.cpu(), cr.grad)
    cos = {n: _cos(params[n].grad.cpu(), pr[n].grad) for n in params if _is_qk(n)}
    nq = max((v / gate[k], v, k) for k, v in worst.items() if not _is_qk(k))
    wq = max(v for k, v in worst.items() if _is_qk(k))
    qk_gate = TOL_QK[dt] if m > 1 else TOL_QK_SIZE
    print(f"[M={m} {dt}] loss {el:.2e} (gate {LOSS_TOL[dt]:.0e}); non-q/k gradients: closest to its gate {nq[1]:.2e} ({nq[2]}, gate "
          f"{gate[nq[2]]:.1e}), worst {max(v for k, v in worst.items() if not _is_qk(k)):.2e}; q/k {wq:.2e} (gate {qk_gate:.0e}, cosine "
          f">= {min(cos.values()):.6f}); d mu {emu:.2e}, d c {ec:.2e}")
    assert el <= LOSS_TOL[dt]
    bad = {k: v for k, v in worst.items() if v > (qk_gate if _is_qk(k) else gate[k])}
    assert not bad, bad
    if m == 1:
        assert min(cos.values()) >= COS_QK_SIZE, cos
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
        eng.train_backward_part(serial, part, B, x.shape[2], *args, stream)
        torch.cuda.synchronize()
        if check is not None:
            check(part, big.cpu())
    return big.cpu(), out.cpu(), gx.cpu(), gmu.cpu(), gc.cpu()


@pytest.mark.grad
@pytest.mark.parametrize("m", WIDTHS)
def test_backward_stays_inside_the_gradient_slices(m, monkeypatch):
    """The backward runs in three parts (st_train_backward_part), each writing the gradients of its own parameters.  After part p,
    every float of a caller-owned gradient buffer outside the slices of the parameters of parts 0..p -- the slices of later parts, the
    64-byte alignment gaps and a 1 MB tail guard -- still holds the sentinel.  At the end each slice equals the gradient the autograd
    path produced, and the single-stream order (ST_TRAIN_SIDE=0) gives the same buffer bit for bit.  (final_proj's weight gradient on
    the TN path stored whole 64-column tiles: at M = 200 rows 200..255 of a 200-row slice, into in_proj.weight's slice -- which part 2
    overwrites later, so only a check between the parts sees it, whatever the timing of the side stream.)"""
    inp = make_inputs(B, T, seed=300 + m, lengths=LENGTHS, n_feats=m)
    t = torch.tensor([0.2, 0.5, 0.8], device="cuda")
    gen = torch.Generator().manual_seed(400 + m)
    g = (torch.randn(B, m, T, generator=gen) * inp["mask"]).cuda()

    dec = _decoder(m, "f16")
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
        print(f"[M={m}] after backward part {part}: {stray.numel()} floats written outside the slices of parts 0..{part}"
              + (f" ({int(stray[0])}..{int(stray[-1])}; inside {where})" if stray.numel() else ""))
        assert stray.numel() == 0, (part, where)

    monkeypatch.delenv("ST_TRAIN_SIDE", raising=False)
    res = _backward_into_own_buffer(dec, t, inp, g, check)
    big = res[0]
    print(f"[M={m}] flat gradient buffer: {n} floats, {int((~written[2][:n]).sum())} of them gaps, {GUARD} guard")
    for name, (off, k, shape) in slices.items():
        assert torch.equal(big[off:off + k].view(shape), want[name]), name
    for a, b in zip(res[1:], want_in):
        assert torch.equal(a, b)

    monkeypatch.setenv("ST_TRAIN_SIDE", "0")          # read when the engine first trains: a fresh decoder
    dec1 = _decoder(m, "f16")
    res1 = _backward_into_own_buffer(dec1, t, inp, g, check)
    assert torch.equal(res1[0].view(torch.int32), big.view(torch.int32))
    for a, b in zip(res1[1:], res[1:]):
        assert torch.equal(a, b)
