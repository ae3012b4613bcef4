"""Decoder filter widths, gin widths and depths other than the default (F = 1024, G = 256, L = 6) against the fp32 oracle on a
real MI355X.  Run with ``-m gpu``.  The oracle itself is pinned to the reference at such configs by test_oracle_golden.py
(tests/golden/config_outputs.npz).

  case       F     G     L   why
  F128       128   256   6   two-kernel FFN (F % 256 != 0), 128-wide conv tiles for cond_proj.0 / .2 and ffn1, fallback weight
                             gradients with cout16 = F -- ffn1's (3C = 768 frames) larger than 3F
  F384       384   256   6   as F128, with several 128-wide column tiles
  F2304      2304  256   6   fused FFN off although F % 256 == 0 (F > 2048); the largest weight-gradient partials (F^2)
  F256-M300  256   256   6   final_proj's fallback weight gradient with cout16 = Mp = 384 > F
  G4         1024  4     6   adaLN_modulation.0 over a 4-wide k chunk (inference linear, training linear_multi, its gradient)
  G260       1024  260   6   a 256-wide and a partial 4-wide k chunk; CFG's fake speaker of width G
  G1024      1024  1024  6   four full k chunks
  L2         1024  256   2   one long skip; block 0 the only first-half block; one block per backward part
  L16        1024  256   16  the most blocks training accepts: 8 skip buffers, the longest backward parts

The evaluation / solve, loss / gradient and bounds checks are those of test_gpu_channel_widths.py (decoder_checks.py), at its
shapes (B = 3, T = 130 ragged) and gates.  The at-size test runs the shipped tile policy at R = B * T = 12000 rows, where the
weight-gradient splits need their full scratch: before the scratch was sized by the largest operand wgrad() is called with, the
backward of F128 and F256-M300 failed there with "weight-gradient scratch too small".  Its gates are test_gpu_training.py's at
size: 3e-3 of max |ref| for every tensor but the q / k projections, 8e-2 and cosine 0.999 for those, with the matched-operand
check below.

The q / k projections' gradients are ill-conditioned in the attention operands at random init (test_gpu_training.py).  Every case
therefore also holds them to the oracle evaluated at the native forward's own q, k and v (decoder_checks.check_qk_matched, gate
TOL_QK_MATCHED), which leaves the native backward chain compared end to end, and to a cosine.  F2304 (f16, 1.2e-2), L16 (f16,
1.3e-2) and G260 (bf16, 1.4e-1) exceed the small-shape end-to-end gate TOL_QK (1e-2 / 1e-1); for those three alone the end-to-end
gate is test_gpu_training.py's at-size one (8e-2 / 3e-1) -- as there, only together with the matched-operand check.
"""
import functools

import pytest
import torch

import oracle
from oracle.inputs import make_inputs
from decoder_checks import (B, COS_QK_SIZE, LENGTHS, LOSS_TOL, T, TOL, TOL_QK_SIZE, check_backward_bounds, check_evaluation_and_solve,
                            check_loss_and_gradients, check_qk_matched, cos, is_qk, native_qkv, rel)

pytestmark = pytest.mark.gpu

# name: (filter_channels, gin_channels, n_layers, mel channels, seed)
CONFIGS = {
    "F128": (128, 256, 6, 128, 11),
    "F384": (384, 256, 6, 128, 12),
    "F2304": (2304, 256, 6, 128, 13),
    "F256-M300": (256, 256, 6, 300, 14),
    "G4": (1024, 4, 6, 128, 15),
    "G260": (1024, 260, 6, 128, 16),
    "G1024": (1024, 1024, 6, 128, 17),
    "L2": (1024, 256, 2, 128, 18),
    "L16": (1024, 256, 16, 128, 19),
}
BF16 = ["F384", "G260", "L2"]
CASES = [(n, "f16") for n in CONFIGS] + [(n, "bf16") for n in BF16]
# End to end, the q / k gradients of these cases exceed TOL_QK; they are held to the at-size gate, with the matched-operand check
# that every case runs (module docstring).
QK_AT_SIZE = {("F2304", "f16"), ("L16", "f16"), ("G260", "bf16")}
AT_SIZE = ["F128", "F384", "F2304", "F256-M300"]
SIZE_B, SIZE_T = 12, 1000          # R = 12000 padded rows; more items rather than longer ones (the oracle keeps B H T^2 scores per layer)


def _config(name):
    f, g, n_layers, m, _ = CONFIGS[name]
    return oracle.DecoderConfig(noise_channels=m, cond_channels=m, out_channels=m, filter_channels=f, gin_channels=g, n_layers=n_layers)


@functools.lru_cache(maxsize=None)
def _state_dict(name):
    return oracle.make_state_dict(800 + CONFIGS[name][4], _config(name))


def _decoder(name, dt):
    from stabletts_amd.flow_matching import CFMDecoder
    cf = _config(name)
    m = cf.noise_channels
    d = CFMDecoder(m, m, 256, m, cf.filter_channels, 4, cf.n_layers, 3, 0.1, cf.gin_channels, operand_dtype=dt)
    d.estimator.load_state_dict(_state_dict(name))
    return d.cuda().eval()


def _inputs(name, seed, b=B, t=T, **kw):
    cf = _config(name)
    return make_inputs(b, t, seed=seed, n_feats=cf.noise_channels, gin=cf.gin_channels, **kw)


@pytest.mark.parametrize("name,dt", CASES)
def test_evaluation_and_solve_vs_oracle(name, dt):
    s = CONFIGS[name][4]
    inp = _inputs(name, s, lengths=LENGTHS)
    fs, fc = oracle.make_cfg_params(4321 + s, _config(name))
    check_evaluation_and_solve(name, _decoder(name, dt), _state_dict(name), inp, fs, fc, dt)


@pytest.mark.grad
@pytest.mark.parametrize("name,dt", CASES)
def test_loss_and_every_gradient_vs_oracle_autograd(name, dt):
    s = CONFIGS[name][4]
    m = _config(name).noise_channels
    inp = _inputs(name, 100 + s, lengths=LENGTHS)
    x1 = _inputs(name, 200 + s)["z"]
    g0 = torch.Generator().manual_seed(s)
    t_rand = torch.rand(B, 1, 1, generator=g0)
    z = torch.randn(B, m, T, generator=g0)
    check_loss_and_gradients(name, _decoder(name, dt), _state_dict(name), inp, x1, t_rand, z, dt, qk_at_size=(name, dt) in QK_AT_SIZE)


@pytest.mark.grad
@pytest.mark.parametrize("name", list(CONFIGS))
def test_backward_stays_inside_the_gradient_slices(name, monkeypatch):
    """decoder_checks.check_backward_bounds: nothing outside the parameter slices of parts 0..p changes after backward part p, the
    slices equal the autograd gradients, and ST_TRAIN_SIDE=0 gives the same buffer bit for bit."""
    s = CONFIGS[name][4]
    m = _config(name).noise_channels
    inp = _inputs(name, 300 + s, lengths=LENGTHS)
    t = torch.tensor([0.2, 0.5, 0.8], device="cuda")
    gen = torch.Generator().manual_seed(400 + s)
    g = (torch.randn(B, m, T, generator=gen) * inp["mask"]).cuda()
    check_backward_bounds(name, lambda: _decoder(name, "f16"), inp, t, g, monkeypatch)


@functools.lru_cache(maxsize=None)
def _size_case(name):
    """One compute_loss step at B = 12 x T = 1000 (ragged) through the ORACLE's autograd (fp32 CPU): loss, every parameter gradient,
    d loss / d mu, d loss / d c."""
    s = CONFIGS[name][4]
    m = _config(name).noise_channels
    inp = _inputs(name, 500 + s, SIZE_B, SIZE_T, ragged=True)
    x1 = _inputs(name, 600 + s, SIZE_B, SIZE_T)["z"]
    g0 = torch.Generator().manual_seed(700 + s)
    t_rand = torch.rand(SIZE_B, 1, 1, generator=g0)
    z = torch.randn(SIZE_B, m, SIZE_T, generator=g0)
    with torch.enable_grad():
        pr = {k: v.clone().requires_grad_(True) for k, v in _state_dict(name).items()}
        mu = inp["mu"].clone().requires_grad_(True)
        c = inp["c"].clone().requires_grad_(True)
        loss, _ = oracle.compute_loss(pr, x1, inp["mask"], mu, c, t_rand, z)
        loss.backward()
    return dict(inp=inp, x1=x1, t_rand=t_rand, z=z, loss=float(loss.detach()), gmu=mu.grad, gc=c.grad,
                grads={k: v.grad for k, v in pr.items()})


@pytest.mark.grad
@pytest.mark.parametrize("name", AT_SIZE)
def test_gradients_at_size(name):
    """f16 loss and every gradient at R = 12000 padded rows with the tile policy as shipped (no ST_* override) against the oracle's
    autograd on the same inputs.  The weight-gradient splits fill their scratch here; at B = 3 x T = 130 they never come close."""
    sc = _size_case(name)
    inp = sc["inp"]
    dec = _decoder(name, "f16")
    eng = dec.estimator.engine()
    mu = inp["mu"].cuda().requires_grad_(True)
    c = inp["c"].cuda().requires_grad_(True)
    eng.debug_capture(True)
    try:
        loss, _ = dec.compute_loss(sc["x1"].cuda(), inp["mask"].cuda(), mu, c, t_rand=sc["t_rand"].cuda(), z=sc["z"].cuda())
        loss.backward()
        torch.cuda.synchronize()
        subst = native_qkv(eng, SIZE_B, SIZE_T, _config(name).n_layers)
    finally:
        eng.debug_capture(False)
    params = dict(dec.estimator.named_parameters())
    assert set(params) == set(sc["grads"])
    for n, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    worst = {n: rel(params[n].grad.cpu(), sc["grads"][n]) for n in params}
    cs = {n: cos(params[n].grad.cpu(), sc["grads"][n]) for n in params if is_qk(n)}
    el = abs(float(loss.detach()) - sc["loss"]) / sc["loss"]
    emu, ec = rel(mu.grad.cpu(), sc["gmu"]), rel(c.grad.cpu(), sc["gc"])
    wo = max((v, k) for k, v in worst.items() if not is_qk(k))
    wq = max(v for k, v in worst.items() if is_qk(k))
    print(f"[{name} f16] B={SIZE_B} T={SIZE_T} ragged ({int(inp['lengths'].sum())} valid frames): loss {el:.2e} (gate {LOSS_TOL['f16']:.0e}); "
          f"worst non-q/k {wo[0]:.2e} ({wo[1]}, gate {TOL['f16']:.0e}); q/k {wq:.2e} (gate {TOL_QK_SIZE['f16']:.0e}), min cosine "
          f"{min(cs.values()):.6f} (gate {COS_QK_SIZE['f16']}); d mu {emu:.2e}, d c {ec:.2e}")
    check_qk_matched(name, subst, params, _state_dict(name), sc["x1"], inp, sc["t_rand"], sc["z"], "f16")
    assert el <= LOSS_TOL["f16"]
    bad = {k: v for k, v in worst.items() if v > (TOL_QK_SIZE["f16"] if is_qk(k) else TOL["f16"])}
    assert not bad, bad
    assert min(cs.values()) >= COS_QK_SIZE["f16"], cs
    assert emu <= TOL["f16"] and ec <= TOL["f16"], (emu, ec)
