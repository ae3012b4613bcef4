"""The proposed decoder mode "split_input" ("split", plus the LayerNorm output h1 and the attention output ao as
hi + lo operand pairs) as far as a CPU can say: the arithmetic of a hi + lo operand pair in float64, and the CPU emulation
(attn_split_input_emul.py) pinned against the published h1 figures, with the gain it predicts for the mode.  The mode itself is not
built; these are the numbers a build is to be held against."""
import pytest
import torch

import attn_split_input_emul as em
from oracle.inputs import make_inputs

def test_pair_arithmetic_in_float64():
    """What a GEMM over operand pairs computes, restated in float64 (every product of two f16 values is exact there): with hi = fl16(x),
    lo = fl16(x - hi) on both sides, W_hi x_hi + W_hi x_lo + W_lo x_hi against the float64 product W x at C = 256.  x has the magnitude
    of a modulated LayerNorm output (unit variance, scale 1 + N(0, 0.15), shift N(0, 0.15)), W the Xavier range of the 256 -> 256
    projections.  Dropped: W_lo x_lo (2^-22 per term) and the pairs' own residuals (2^-22 relative; 2^-25 absolute where lo is a
    subnormal f16, which W's is) -- a few 2^-22 of the largest output in all, so 2^-19 holds with room; a single f16 operand gives
    2^-11.  This is the step the emulation takes for granted when it treats a pair as hi + lo."""
    g = torch.Generator().manual_seed(5)
    C, T = 256, 512
    x = torch.randn(C, T, generator=g) * (1 + 0.15 * torch.randn(C, 1, generator=g)) + 0.15 * torch.randn(C, 1, generator=g)
    w = (torch.rand(C, C, generator=g) * 2 - 1) * (6.0 / (C + C)) ** 0.5
    f16 = lambda v: v.half().double()
    xd, wd = x.double(), w.double()
    x_hi, w_hi = f16(x), f16(w)
    x_lo, w_lo = (xd - x_hi).half().double(), (wd - w_hi).half().double()
    exact = wd @ xd
    got = w_hi @ x_hi + w_hi @ x_lo + w_lo @ x_hi
    single = w_hi @ x_hi
    err = float((got - exact).abs().max() / exact.abs().max())
    err1 = float((single - exact).abs().max() / exact.abs().max())
    print(f"hi + lo pair: {err:.2e} (2^-19 = {2 ** -19:.2e}); single f16 operands: {err1:.2e}")
    assert err <= 2.0 ** -19
    assert err1 > 2.0 ** -16          # the control: the test can tell the two apart
    # the emulation's `pair` is hi + lo
    assert torch.equal(em.pair(x).double(), x_hi + x_lo)


# profiles/r06_h1_rounding_sensitivity.txt, ada 0.15, q/k x3 (tools/h1_rounding_sensitivity.py at B = 2 x T = 1000 ragged)
PUBLISHED = [
    ("h1 -> f16 for q, k only", dict(h1_qk="f16"), 1.85e-3),
    ("h1 -> f16 for v only", dict(h1_v="f16"), 5.3e-4),
    ("h1 + q, k, v -> f16", dict(h1_qk="f16", h1_v="f16", qk="f16", v="f16"), 2.52e-3),
    ("h1 + v -> f16, q, k split", dict(h1_qk="f16", h1_v="f16", v="f16"), 1.89e-3),
]


def test_emulation_reproduces_the_published_h1_figures():
    """The emulation at the tool's own configuration (a few seconds of CPU) against the four figures the tool published, to two digits: half a
    unit of the second significant digit.  (The tool left q and k exact where it says "split"; so does the spec here.)"""
    import math
    inp = make_inputs(2, 1000, seed=81, lengths=[1000, 655])
    t = torch.tensor(0.5)
    sd = em.trained_like(0.15, 3.0)
    ref = em.forward(sd, t, inp)
    bad = []
    for name, spec, pub in PUBLISHED:
        got = em.error(sd, t, inp, spec, ref)
        half_unit = 0.5 * 10.0 ** (math.floor(math.log10(pub)) - 1)
        print(f"{name}: emulation {got:.3e}, published {pub:.2e} (+- {half_unit:.0e})")
        if abs(got - pub) > half_unit:
            bad.append((name, got, pub))
    assert not bad, bad


@pytest.mark.parametrize("shape", ["A", "B"])
def test_emulated_gain_is_large_enough_to_test_at_both_shapes(shape):
    """A GPU test of the mode is to ask the device for half of the gain e(split) - e(split_input) that the emulation predicts in the
    arg-max regime.  That is a test only where the predicted gain is a good part of the error: at least 20 % of e_emul(split) at each
    of the two shapes kept for it."""
    inp = em.shape_inputs(shape)
    t = torch.tensor(0.5)
    sd = em.trained_like(0.15, 3.0)
    ref = em.forward(sd, t, inp)
    e = {m: em.error(sd, t, inp, em.MODES[m], ref) for m in ("16bit", "split", "split_input")}
    print(f"shape {shape}, ada 0.15, q/k x3, emulated: " + ", ".join(f"{m} {v:.2e}" for m, v in e.items()))
    assert e["split"] - e["split_input"] >= 0.2 * e["split"]
