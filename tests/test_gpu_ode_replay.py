"""The native ODE controllers (engine_solve.cpp: solve_adaptive, solve_implicit_adams, step_fixed; adaptive_ode.hip: the norm,
final-sum and dense-output kernels; misc_kernels.hip: lincomb, cfg_combine) against the oracle's drivers replayed over the NATIVE
vector field -- the same function on both sides, so the native solve has to take the replay's decisions exactly and land within
fp32 rounding of it (ode_replay_checks.py: the gate, identical for every case).  test_gpu_parity.py's adaptive and Adams tests
remain the comparison against the fp32 field; nothing here evaluates the CPU oracle's DiT.

Shapes: M = 80 / 200 pad the state to Mp = 128 / 256 channels (the norm's element count B M T against the B T Mp elements it reads);
B = 9 x T = 1000 x 128 is the smallest state above 1024 blocks x 1024 elements (the norm's grid-stride loop wraps, the final kernel
sums 1024 partials); implicit Adams at n = 14 fills its 11-entry history; a zero field takes the h0 = 1e-6 and ratio == 0 branches.
"""
import sys
import types

import pytest
import torch

import oracle
from oracle.inputs import make_inputs

import ode_replay_checks as rc

pytestmark = pytest.mark.gpu

_decoders, _cases = {}, {}
NUDGES = (1, 3)      # patterns of ode_replay_checks.nudged whose fp32-state replays join the precondition
MOVED = (0, 1, 2, 3)      # patterns of ode_replay_checks.moved_start whose float64-state replays join the precondition


def _config(m):
    return oracle.DecoderConfig(noise_channels=m, cond_channels=m, out_channels=m)


def _decoder(m, dt="f16", field="random"):
    """Default decoder config at n_feats = m.  field: 'zero' (final_proj = 0), 'const' (final_proj.weight = 0) or 'random'."""
    from stabletts_amd.flow_matching import CFMDecoder
    key = (m, dt, field)
    if key not in _decoders:
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        sd = dict(oracle.make_state_dict(1234 if m == 128 else 99 if m == 80 else 1000 + m, _config(m)))
        if field != "random":
            sd["final_proj.weight"] = torch.zeros_like(sd["final_proj.weight"])
        if field == "zero":
            sd["final_proj.bias"] = torch.zeros_like(sd["final_proj.bias"])
        d = CFMDecoder(m, m, 256, m, 1024, 4, 6, 3, 0.1, 256, operand_dtype=dt)
        d.estimator.load_state_dict(sd)
        _decoders[key] = (d.to("cuda:0").eval(), sd)
    return _decoders[key]


def _cfg_kwargs(m, strength):
    if strength is None:
        return None
    fs, fc = oracle.make_cfg_params(4321 if m == 128 else 4321 + m, _config(m))
    return dict(fake_speaker=fs.cuda(), fake_content=fc.cuda(), cfg_strength=strength)


def _case(label, method, m, B, T, lengths, seed, n=10, cfg=None, dt="f16", field="random"):
    """The native solve and the replays of one case, computed once per process: (inp, out, native stats, r32, r64, nudged replays, moved-start replays)."""
    if label not in _cases:
        dec, _ = _decoder(m, dt, field)
        inp = {k: v.cuda() for k, v in make_inputs(B, T, seed=seed, lengths=lengths, n_feats=m).items() if k != "lengths"}
        kw = _cfg_kwargs(m, cfg)
        out = dec(inp["mu"], inp["mask"], n, 1.0, inp["c"], method, kw, z=inp["z"])
        st = dec.estimator.engine().last_solve_stats()
        f = rc.native_field(dec, inp, kw)
        r32 = rc.replay(method, f, inp["z"], n, torch.float32)
        r64 = rc.replay(method, f, inp["z"], n, torch.float64)
        nudges = () if method in rc.FIXED else tuple(rc.replay(method, rc.nudged(f, k), inp["z"], n, torch.float32) for k in NUDGES)
        moved = () if method in rc.FIXED else tuple(rc.replay(method, f, rc.moved_start(inp["z"], k), n, torch.float64) for k in MOVED)
        _cases[label] = (inp, out, st, r32, r64, nudges, moved)
    return _cases[label]


def _check(label, method, *a, margin=True, check_stats=True, fallback=None, **k):
    inp, out, st, r32, r64, nudges, moved = _case(label, method, *a, **k)
    res = rc.compare(out, st, r32, r64, inp["mask"], "dopri5" if method is None else method, label, margin=margin,
                     check_stats=check_stats, fallback=fallback, nudges=nudges, moved=moved)
    pad = ~inp["mask"].bool().expand_as(out)
    if pad.any():
        assert torch.equal(out[pad], inp["z"][pad])      # the field is exactly 0 on padded frames at every stage
    return res


# the adaptive pairs' cases at M = 80; their largest yardstick stands in where a case's own is exactly 0 (the zero field)
M80_DOPRI5 = ("dopri5 M=80 B=2 T=50", "dopri5", 80, 2, 50, [50, 31], 8)
# Input seeds of the B = 1, T = 12 cases: 31 (test_gpu_parity.py's) unless it fails the precondition, then the first seed after it
# that meets it.  fehlberg2 M = 80: at 31 and 33 a nudged replay takes another sequence (17 / 1 against 19 / 2 rejections with every
# ratio 3e-2 from 1), and at 32 float64-state replays from z moved by one fp32 ulp land up to 1.3e-2 from the plain one, 11 yardsticks
# (the native solve, with the replay's 17 steps and 2 rejections, is 1.155e-2 away there: the same spread).  adaptive_heun takes ~900 steps whose ratios
# crowd around 1: of the seeds 31 ... 150 only 49, 66, 84 (M = 128) and 44, 77, 78 (M = 80) keep all of them 1e-3 away, and at 49 a
# nudged replay takes another sequence.
# Finding a seed again (a change of the estimator's rounding can move a ratio across the margin; the controller is not wrong then and
# compare() says "choose another seed"): run _check(*_small(solver, m)) with SMALL_SEEDS[(solver, m)] = 31, 32, ... and keep the first
# seed whose failure is NOT one of the "choose another seed" assertions -- those depend on the replays alone, so the native result has
# no say in the choice.  A replay aborts cheaply if odeint_adaptive's log raises on the first |ratio - 1| < 1e-3; 120 seeds take ~30 s.
SMALL_SEEDS = {("fehlberg2", 80): 34, ("adaptive_heun", 128): 66, ("adaptive_heun", 80): 44}


def _small(solver, m):
    return (f"{solver} M={m} B=1 T=12", solver, m, 1, 12, [12], SMALL_SEEDS.get((solver, m), 31))


M80_SMALL = {s: _small(s, 80) for s in ("bosh3", "fehlberg2", "adaptive_heun")}


def _m80_yardstick():
    ys = []
    for args in (M80_DOPRI5, *M80_SMALL.values()):
        inp, _, _, r32, r64 = _case(*args)[:5]
        ys.append(rc.yardstick(r32, r64, inp["mask"]))
    return tuple(max(y[i] for y in ys) for i in range(2))


# ---------------------------------------------------------------- adaptive pairs
@pytest.mark.parametrize("dt,solver,seed", [("f16", None, 24), ("bf16", "dopri5", 25)])
def test_dopri5_m128_cfg_rejects_and_overshoots(dt, solver, seed):
    """test_gpu_parity.py's dopri5 case (B = 2, T = 33, lengths [33, 30], CFG 2.0): it rejects steps, so the rejected-step path is in
    the decision check, and its last step overshoots t = 1.  With CFG 2.0 this case's yardstick (4.9e-4 with f16 operands: a flipped
    16-bit rounding inside the field) is larger than what the overshoot of its last step is worth, so a wrong dense-output ARGUMENT
    is not visible here; the M = 80 and M = 200 cases below assert the overshoot too and do see it.  (bf16: at that test's seed 24
    the nudged replays take 72 steps against 71; 25 is the next seed that meets the precondition.)"""
    label = f"dopri5 M=128 B=2 T=33 cfg {dt}"
    res = _check(label, solver, 128, 2, 33, [33, 30], seed, cfg=2.0, dt=dt)
    r64 = _cases[label][4]
    assert res["replay"]["rejects"] >= 1 and r64.stats["interp_x"] < 1.0, r64.stats


def test_dopri5_m80_padded_channels():
    """Mp = 128 > M = 80: the norm reads B T Mp elements, 3 / 8 of them zero padding, and divides by B M T.  The last step overshoots
    t = 1 and the yardstick (7e-6) is far below the overshoot: the dense output's argument is in the accuracy gate."""
    _check(*M80_DOPRI5)
    assert _cases[M80_DOPRI5[0]][4].stats["interp_x"] < 1.0


def test_dopri5_m200_padded_channels_cfg():
    """Mp = 256 > M = 200, with CFG; the last step overshoots t = 1 as well."""
    label = "dopri5 M=200 B=2 T=40 cfg"
    _check(label, "dopri5", 200, 2, 40, [40, 27], 12, cfg=2.0)
    assert _cases[label][4].stats["interp_x"] < 1.0


@pytest.mark.parametrize("m", [128, 80])
@pytest.mark.parametrize("solver", ["bosh3", "fehlberg2", "adaptive_heun"])
def test_other_pairs(solver, m):
    """fehlberg2 and adaptive_heun are not FSAL: y1 is a combination of its own and the derivative carried into the next step is
    k[S], swapped into k[0].  bosh3's dense output takes its f1 from slot 6 of the interpolation kernel."""
    _check(*_small(solver, m))


def test_dopri5_state_above_the_norm_grid():
    """B = 9 x T = 1000 x 128 = 1 152 000 elements: the norm runs its 1024-block cap, 101 blocks take a second pass of the
    grid-stride loop and the final kernel sums 1024 partials, four per thread."""
    _check("dopri5 M=128 B=9 T=1000 cfg", "dopri5", 128, 9, 1000, [1000, 910, 820, 740, 650, 560, 470, 380, 300], 44, cfg=2.0)


@pytest.mark.parametrize("solver", ["dopri5", "bosh3", "fehlberg2", "adaptive_heun"])
def test_zero_field(solver):
    """final_proj = 0: d1 = 0 takes h0 = 1e-6, every error ratio is 0 and takes the tenfold growth: exactly 7 steps, no
    rejection.  The output is the interpolant of a constant, z up to its rounding."""
    res = _check(f"{solver} M=80 zero field", solver, 80, 2, 20, [20, 13], 8, field="zero", margin=False, fallback=_m80_yardstick())
    assert res["native"] == dict(nfe=2 + rc.STAGES[solver] * 7, steps=7, rejects=0), res["native"]
    assert res["replay"]["h0"] == 1e-6


@pytest.mark.parametrize("solver", ["dopri5", "bosh3", "fehlberg2", "adaptive_heun"])
def test_constant_field(solver):
    """final_proj.weight = 0: the field is the bias on every valid frame, whatever the state; the solution is z + bias, and the
    native result is within 4 fp32 roundings (4 x 2^-24 max|z + bias|) of it on the valid frames.  Measured: 2.9 / 1.7 / 3.7 / 2.9
    for dopri5 / bosh3 / fehlberg2 / adaptive_heun, where the fp32 replay of torchdiffeq's literal dense-output formula is 1.3 / 8.3 /
    3.6 / 3.6 away; with that literal form the native kernel measured 2.9 / 6.0 / 5.9 / 2.5 (adaptive_ode.hip now forms the
    polynomial's coefficients from the increments y1 - y0 and y_mid - y0)."""
    label = f"{solver} M=80 constant field"
    res = _check(label, solver, 80, 2, 20, [20, 13], 8, field="const", fallback=_m80_yardstick())
    inp, out, _, r32, r64 = _cases[label][:5]
    bias = _decoder(80, "f16", "const")[1]["final_proj.bias"].cuda()
    want = (inp["z"].double() + bias.double()[None, :, None]) * inp["mask"].double()
    valid = inp["mask"].bool().expand_as(out)
    dev = float(((out.double() - want) * inp["mask"])[valid].abs().max())
    d32 = float(((r32.out.double() - want) * inp["mask"])[valid].abs().max())
    d64 = float(((r64.out - want) * inp["mask"])[valid].abs().max())
    one = 2.0 ** -24 * float(want.abs().max())      # one fp32 rounding at the largest value
    print(f"{label}: native {dev / one:.1f}, fp32 replay {d32 / one:.1f}, float64 replay {d64 / one:.3f} roundings from z + bias ({res['replay']})")
    assert dev <= 4 * one, (dev / one, d32 / one)


# ---------------------------------------------------------------- implicit Adams
@pytest.mark.parametrize("m,n,cfg,seed", [(128, 10, None, 37), (128, 6, 2.0, 38), (80, 14, None, 37)])
def test_implicit_adams(m, n, cfg, seed):
    """nfe and the number of unconverged steps equal the replay's.  n = 14: from step 12 on the history holds its 11 entries and
    the oldest buffer is recycled for the new sample.  (Seed 37 is test_gpu_parity.py's; with CFG at n = 6 two of the replays from
    a start moved by one fp32 ulp take a corrector iteration more there, 38 is the next seed that meets the precondition.)"""
    res = _check(f"implicit_adams M={m} n={n}" + (" cfg" if cfg else ""), "implicit_adams", m, 2, 40, [40, 29], seed, n=n, cfg=cfg)
    assert res["native"]["steps"] == n


# ---------------------------------------------------------------- fixed grid
@pytest.mark.parametrize("solver", ["euler", "midpoint", "rk4"])
def test_fixed_grid(solver):
    """The fused Euler update of the CFG combine, the 3/8-rule coefficients and the stage times, at fp32 level."""
    _check(f"{solver} M=80 B=3 n=4 cfg", solver, 80, 3, 30, [30, 21, 9], 52, n=4, cfg=2.0, check_stats=False)


# ---------------------------------------------------------------- Python driver path
@pytest.mark.parametrize("which", ["m80", "m128 cfg"])
def test_python_driver_path_gives_the_fp32_replay_bit_for_bit(monkeypatch, which):
    """A solver name outside _lib.SOLVERS hands the time stepping to torchdiffeq.odeint around the native estimator
    (CFMDecoder._solve_with_torchdiffeq).  With odeint = the oracle's dopri5 driver that is the fp32 replay itself."""
    seen = {}

    def odeint(fn, y0, t, method=None, rtol=None, atol=None):
        seen.update(method=method, rtol=rtol, atol=atol)
        return torch.stack([y0, oracle.odeint_adaptive(fn, y0, "dopri5", float(t[-1]), rtol, atol)])

    fake = types.ModuleType("torchdiffeq")
    fake.odeint = odeint
    monkeypatch.setitem(sys.modules, "torchdiffeq", fake)
    if which == "m80":
        args, m, cfg = M80_DOPRI5, 80, None
    else:
        args, m, cfg = ("dopri5 M=128 B=2 T=33 cfg f16", None, 128, 2, 33, [33, 30], 24), 128, 2.0
    inp, _, _, r32 = _case(*args, **({"cfg": cfg} if cfg else {}))[:4]
    dec, _ = _decoder(m)
    out = dec(inp["mu"], inp["mask"], 10, 1.0, inp["c"], "dopri5_via_python", _cfg_kwargs(m, cfg), z=inp["z"])
    assert seen == dict(method="dopri5_via_python", rtol=1e-5, atol=1e-5)
    assert torch.equal(out, r32.out)
