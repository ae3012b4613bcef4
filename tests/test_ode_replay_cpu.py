"""The replay harness of ode_replay_checks.py without a GPU: the oracle's fp32 estimator stands in for the native field (it takes
y.float() and answers in the state's dtype, exactly like native_field), so the fp32-state and float64-state replays, the decision
log and the gate's arithmetic are tested on the CPU.  The GPU tests (test_gpu_ode_replay.py) put the native solve through the
same functions."""
import pytest
import torch

import oracle
from oracle.inputs import make_inputs

import ode_replay_checks as rc

CFG80 = oracle.DecoderConfig(noise_channels=80, cond_channels=80, out_channels=80)


def _field(sd, inp):
    def f(t, y):
        return oracle.decoder_forward(sd, torch.as_tensor(t, dtype=torch.float32), y.float(), inp["mask"], inp["mu"], inp["c"]).to(y.dtype)
    return f


@pytest.fixture(scope="module")
def sd80():
    return oracle.make_state_dict(99, CFG80)


@pytest.fixture(scope="module")
def dopri5_m80(sd80):
    inp = make_inputs(2, 20, seed=8, lengths=[20, 13], n_feats=80)
    f = _field(sd80, inp)
    return inp, rc.replay("dopri5", f, inp["z"], 10, torch.float32), rc.replay(None, f, inp["z"], 10, torch.float64), f


def test_fp32_and_float64_state_replays_take_one_sequence(dopri5_m80):
    """M = 80, B = 2, T = 20, lengths [20, 13], dopri5: identical sequences, fp32's distance from float64 below 1e-6 of max|out|,
    every error ratio further than 1e-3 from 1.  Measured: 54 steps, 3 rejections, nfe 326 on both; 3.7e-7; closest ratio 0.059 away."""
    inp, r32, r64, _ = dopri5_m80
    assert r32.out.dtype == torch.float32 and r64.out.dtype == torch.float64
    assert rc.decisions(r32) == rc.decisions(r64)
    assert {k: r32.stats[k] for k in ("nfe", "steps", "rejects")} == {k: r64.stats[k] for k in ("nfe", "steps", "rejects")}
    assert r64.stats["rejects"] >= 1 and r64.stats["nfe"] == 2 + 6 * r64.stats["steps"]
    yard = float((r32.out.double() - r64.out).abs().max() / r64.out.abs().max())
    margin = min(rc.threshold_margin(r32), rc.threshold_margin(r64))
    print(f"replays: {r64.stats}; fp32 vs float64 state {yard:.2e} of max|out|; closest error ratio to 1: {margin:.3f} away")
    assert yard < 1e-6 and margin > 1e-3


def test_decision_log_has_one_entry_per_step(dopri5_m80):
    _, r32, r64, _ = dopri5_m80
    for r in (r32, r64):
        assert len(r.log) == r.stats["steps"]
        assert sum(1 for v in r.log if v > 1.0) == r.stats["rejects"]
        assert 0.0 < r.stats["interp_x"] <= 1.0


def test_compare_accepts_the_fp32_replay_and_rejects_a_wrong_controller(dopri5_m80):
    """The gate on itself: the fp32 replay as the 'native' result passes (ratio 1); the same output with one step more, or an output
    5 yardsticks away, does not."""
    inp, r32, r64, f = dopri5_m80
    st = {k: r32.stats[k] for k in ("nfe", "steps", "rejects")}
    res = rc.compare(r32.out, st, r32, r64, inp["mask"], "dopri5", "cpu-m80")
    assert res["ratio"] == (1.0, 1.0)
    with pytest.raises(AssertionError):
        rc.compare(r32.out, dict(st, steps=st["steps"] + 1, nfe=st["nfe"] + 6), r32, r64, inp["mask"], "dopri5", "cpu-m80-steps")
    off = r64.out + 5.0 * res["yardstick"][0] * inp["mask"]
    with pytest.raises(AssertionError):
        rc.compare(off, st, r32, r64, inp["mask"], "dopri5", "cpu-m80-off")
    # the precondition's conditioning part: a float64-state replay from a start one fp32 ulp away stays within the gate here, and a
    # case where it would not is refused whatever the native result
    moved = rc.replay("dopri5", f, rc.moved_start(inp["z"], 0), 10, torch.float64)
    assert rc.compare(r32.out, st, r32, r64, inp["mask"], "dopri5", "cpu-m80-moved", moved=(moved,))["spread"] <= 4 * res["yardstick"][1]
    with pytest.raises(AssertionError, match="choose another seed"):
        rc.compare(r32.out, st, r32, r64, inp["mask"], "dopri5", "cpu-m80-ill", moved=(rc.Replay(off, r64.stats, r64.log),))


@pytest.mark.parametrize("method", ["dopri5", "bosh3", "fehlberg2", "adaptive_heun"])
def test_zero_field_step_counts(sd80, method):
    """final_proj = 0: the field is identically zero, every error ratio is 0, the step grows tenfold from h0 = 1e-6 (the d0 / d1
    branch of the initial step): exactly 7 steps, no rejection, nfe = 2 + stages * 7 = 44 / 23 / 16 / 9."""
    sd0 = dict(sd80)
    sd0["final_proj.weight"] = torch.zeros_like(sd80["final_proj.weight"])
    sd0["final_proj.bias"] = torch.zeros_like(sd80["final_proj.bias"])
    inp = make_inputs(1, 6, seed=3, n_feats=80)
    for dtype in (torch.float32, torch.float64):
        r = rc.replay(method, _field(sd0, inp), inp["z"], 10, dtype)
        assert r.stats["steps"] == 7 and r.stats["rejects"] == 0 and r.stats["nfe"] == 2 + rc.STAGES[method] * 7
        assert r.stats["h0"] == 1e-6 and r.log == [0.0] * 7
        # the dense output's coefficients cancel exactly in float64 (18 z + 14 z - 32 z with fp32-valued z); in fp32 each of those
        # terms is rounded once, at most (18 + 14 + 32) half-ulps of |z| together
        dev = float((r.out.double() - inp["z"].double()).abs().max())
        assert dev <= (0.0 if dtype == torch.float64 else 64 * 2.0 ** -24 * float(inp["z"].abs().max())), dev


def test_implicit_adams_log_has_one_entry_per_corrector_iteration(sd80):
    inp = make_inputs(1, 6, seed=4, n_feats=80)
    n = 5
    r = rc.replay("implicit_adams", _field(sd80, inp), inp["z"], n, torch.float32)
    # two Runge-Kutta start-up steps (4 evaluations each), then one evaluation per step plus one per corrector iteration
    assert r.stats["steps"] == n and len(r.log) == r.stats["nfe"] - 8 - (n - 2)
    assert n - 2 <= len(r.log) <= 4 * (n - 2)
    assert r.stats["rejects"] <= sum(1 for v in r.log if not v < 1.0) // 4


def test_fixed_grid_replay_equals_cfm_forward(sd80):
    inp = make_inputs(1, 6, seed=5, n_feats=80)
    for method in rc.FIXED:
        r = rc.replay(method, _field(sd80, inp), inp["z"], 2, torch.float32)
        with torch.inference_mode():
            assert torch.equal(r.out, oracle.cfm_forward(sd80, inp["mu"], inp["mask"], 2, inp["z"], inp["c"], method))
        assert r.log == [] and r.stats["rejects"] == 0
