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
from decoder_checks import B, LENGTHS, T, check_backward_bounds, check_evaluation_and_solve, check_loss_and_gradients

pytestmark = pytest.mark.gpu

WIDTHS = [1, 80, 200, 256, 300, 450]
CASES = [(m, "f16") for m in WIDTHS] + [(200, "bf16"), (300, "bf16")]


def _config(m):
    return oracle.DecoderConfig(noise_channels=m, cond_channels=m, out_channels=m)


@functools.lru_cache(maxsize=None)
def _state_dict(m):
    return oracle.make_state_dict(700 + m, _config(m))


def _decoder(m, dt):
    from stabletts_amd.flow_matching import CFMDecoder
    d = CFMDecoder(m, m, 256, m, 1024, 4, 6, 3, 0.1, 256, operand_dtype=dt)
    d.estimator.load_state_dict(_state_dict(m))
    return d.cuda().eval()


@pytest.mark.parametrize("m,dt", CASES)
def test_evaluation_and_solve_vs_oracle(m, dt):
    inp = make_inputs(B, T, seed=m, lengths=LENGTHS, n_feats=m)
    fs, fc = oracle.make_cfg_params(4321 + m, _config(m))
    check_evaluation_and_solve(f"M={m}", _decoder(m, dt), _state_dict(m), inp, fs, fc, dt)


@pytest.mark.grad
@pytest.mark.parametrize("m,dt", CASES)
def test_loss_and_every_gradient_vs_oracle_autograd(m, dt):
    inp = make_inputs(B, T, seed=100 + m, lengths=LENGTHS, n_feats=m)
    x1 = make_inputs(B, T, seed=200 + m, n_feats=m)["z"]
    g0 = torch.Generator().manual_seed(m)
    t_rand = torch.rand(B, 1, 1, generator=g0)
    z = torch.randn(B, m, T, generator=g0)
    check_loss_and_gradients(f"M={m}", _decoder(m, dt), _state_dict(m), inp, x1, t_rand, z, dt, qk_at_size=m == 1)


@pytest.mark.grad
@pytest.mark.parametrize("m", WIDTHS)
def test_backward_stays_inside_the_gradient_slices(m, monkeypatch):
    """The backward writes nothing outside the parameter slices of a caller-owned flat gradient buffer, after any of its three
    parts, and ST_TRAIN_SIDE=0 gives the same buffer bit for bit (decoder_checks.check_backward_bounds).  (final_proj's weight
    gradient on the TN path stored whole 64-column tiles: at M = 200 rows 200..255 of a 200-row slice, into in_proj.weight's slice
    -- which part 2 overwrites later, so only a check between the parts sees it, whatever the timing of the side stream.)"""
    inp = make_inputs(B, T, seed=300 + m, lengths=LENGTHS, n_feats=m)
    t = torch.tensor([0.2, 0.5, 0.8], device="cuda")
    gen = torch.Generator().manual_seed(400 + m)
    g = (torch.randn(B, m, T, generator=gen) * inp["mask"]).cuda()
    check_backward_bounds(f"M={m}", lambda: _decoder(m, "f16"), inp, t, g, monkeypatch)
