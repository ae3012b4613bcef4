"""Replay of the ODE controllers over ONE vector field, shared by test_gpu_ode_replay.py (the native estimator on the GPU as the
field) and test_ode_replay_cpu.py (the oracle's fp32 estimator as the field, which tests this harness without a GPU).

An adaptive solver reaches nearly the same answer with almost any controller, so comparing a whole native solve with the CPU
oracle's (fp32 field against 16-bit operands, gates 1e-3 ... 3e-2) cannot see a wrong element count in the RMS norm, a dropped term
of the error estimate, a wrong exponent, a wrong carried derivative or a wrong dense-output weight: those change the step sequence,
not the answer.  Here the oracle's drivers (oracle.odeint_adaptive / odeint_implicit_adams / odeint_fixed) are run over the SAME
field the native solve integrates, once with an fp32 state and once with a float64 state:

  1. precondition: the two replays take the same decision sequence and no decision value (error ratio of a step; the corrector's
     largest |dy_old - dy| / tol of an iteration) lies within MARGIN of its threshold 1 -- the sequence is then a property of the
     problem, not of rounding.  Over several hundred steps that margin alone has let a sequence through that one rounding of the
     field changes (adaptive_heun, 924 steps, closest ratio 1.24e-3 from 1), so fp32-state replays over the field moved by one
     fp32 rounding (nudged) must take the same sequence as well.  And the case must be well enough conditioned for gate 3 to mean
     anything: float64-state replays started from z moved by one fp32 ulp (moved_start) must take the same sequence and stay
     within FACTOR yardsticks of the plain one.  fehlberg2's error estimate dt (k2 - k0) / 512 is nearly blind, its steps grow until
     the integration amplifies a rounding 1e5-fold, and at one seed (M = 80, B = 1, T = 12, seed 32) such starts land up to 1.3e-2
     from each other with a yardstick of 1.2e-3: there one fp32 replay's distance is a single draw of a wide distribution and no
     bound for another fp32 implementation, so such a seed is replaced like one that fails the margin;
  2. decisions: the native solve's (nfe, steps, rejects) equal the float64 replay's exactly;
  3. accuracy: max|native - r64| <= FACTOR * max|r32 - r64| on the valid frames and on the whole tensor.  The yardstick is fp32's
     own distance from float64 on this very case (it is NOT a fixed number: a state that differs in its last bit can flip a 16-bit
     rounding inside the field), measured per case and never taken from the native output; FACTOR = 4 is the project's usual margin
     over it.  A yardstick of exactly 0 is replaced by the largest one of the same solver family.
"""
import collections
import os

import torch

import oracle

FACTOR = 4.0          # native error allowed over the fp32-state replay's own distance from the float64-state replay
MARGIN = 1e-3         # no decision value may be this close to its threshold of 1
STAGES = {"dopri5": 6, "bosh3": 3, "fehlberg2": 2, "adaptive_heun": 1}      # field evaluations per step
FIXED = ("euler", "midpoint", "rk4")

Replay = collections.namedtuple("Replay", "out stats log")


def native_field(dec, inp, cfg_kwargs=None):
    """f(t, y) = the native estimator on the GPU (through dec.cfg_wrapper with CFG): y.float() and the time as an fp32 scalar go in,
    the result comes back in y's dtype.  inp: dict of mu, mask, c on the decoder's device."""
    mask, mu, c = inp["mask"], inp["mu"], inp["c"]

    def f(t, y):
        t = torch.as_tensor(t, dtype=torch.float32)
        if cfg_kwargs is None:
            v = dec.estimator(t, y.float(), mask, mu, c)
        else:
            v = dec.cfg_wrapper(t, y.float(), mask, mu, c, cfg_kwargs)
        return v.to(y.dtype)
    return f


def nudged(f, k):
    """f with its values moved by -1, 0 or +1 fp32 roundings (relative 2^-23) in a fixed pseudo-random pattern number k: the same
    field to fp32 accuracy.  A decision sequence that is a property of the problem survives it."""
    def g(t, y):
        v = f(t, y)
        idx = torch.arange(v.numel(), device=v.device).reshape(v.shape)
        s = ((idx * 2654435761 + k * 40503) >> 7) % 3 - 1
        return v * (1.0 + s.to(v.dtype) * 2.0 ** -23)
    return g


def moved_start(z, k):
    """z with its values moved by -1, 0 or +1 fp32 ulps (relative 2^-23) in the fixed pattern number k of nudged()."""
    idx = torch.arange(z.numel(), device=z.device).reshape(z.shape)
    s = ((idx * 2654435761 + k * 40503) >> 7) % 3 - 1
    return z * (1.0 + s.to(z.dtype) * 2.0 ** -23)


def replay(method, f, z, n, dtype):
    """The oracle driver of `method` (None = dopri5, the reference default) over the field f with the state in `dtype`.  Returns
    Replay(out, stats, log): stats has nfe, steps, rejects (adaptive pairs also h0 and interp_x, the dense output's argument); log has
    one decision value per step (adaptive pairs: the error ratio) or per corrector iteration (implicit Adams), empty for fixed grids."""
    method = "dopri5" if method is None else method
    y0 = z.to(dtype)
    stats, log = {}, []
    with torch.inference_mode():
        if method in oracle.ADAPTIVE_TABLEAUS:
            out = oracle.odeint_adaptive(f, y0, method, stats=stats, log=log)
        elif method == "implicit_adams":
            out = oracle.odeint_implicit_adams(f, y0, oracle.linspace_f32(n), stats=stats, log=log)
        else:
            out = oracle.odeint_fixed(f, y0, oracle.linspace_f32(n), method)
            per = {"euler": 1, "midpoint": 2, "rk4": 4}[method]
            stats.update(nfe=per * n, steps=n, rejects=0)
    return Replay(out, stats, log)


def decisions(r):
    """What the controller decided at every logged value: True = accepted / converged."""
    return [v <= 1.0 for v in r.log] if "h0" in r.stats else [v < 1.0 for v in r.log]


def threshold_margin(r):
    """Smallest distance of a logged decision value from its threshold 1 (inf for an empty log)."""
    return min((abs(v - 1.0) for v in r.log), default=float("inf"))


def _err(a, b, sel=None):
    d = (a.double() - b.double()).abs()
    return float((d if sel is None else d[sel]).max())


def yardstick(r32, r64, mask=None):
    """fp32's own distance from float64 on this case: max|r32 - r64| on the valid frames and on the whole tensor."""
    o32, o64 = r32.out.detach().cpu(), r64.out.detach().cpu()
    valid = None if mask is None else mask.detach().cpu().bool().expand_as(o32)
    return (_err(o32, o64, valid), _err(o32, o64))


def compare(native_out, native_stats, r32, r64, mask=None, method="dopri5", label=None, margin=True, check_stats=True,
            fallback=None, nudges=(), moved=()):
    """The gate of the module docstring.  native_out (B, M, T) on any device, native_stats = last_solve_stats(); r32 / r64 = replay()
    with fp32 / float64 state; mask (B, 1, T) selects the valid frames (None: all).  margin=False drops the threshold margin of the
    precondition (a zero field: every ratio is 0), check_stats=False drops gate 2 (fixed grids have no decisions); fallback = the
    largest yardstick() pair of the same solver family, used where this case's own is exactly 0; nudges = fp32-state replays over
    nudged() fields, which the precondition holds to the same decision sequence; moved = float64-state replays from moved_start()
    points, which it holds to that sequence and to FACTOR yardsticks from r64.  Prints one report
    line, appends it to the file named by ODE_REPLAY_REPORT if set, and returns the measured figures."""
    out = native_out.detach().cpu()
    o64 = r64.out.detach().cpu()
    valid = None if mask is None else mask.detach().cpu().bool().expand_as(out)
    yard = yardstick(r32, r64, mask)
    err = (_err(out, o64, valid), _err(out, o64))
    used = tuple(y if y > 0.0 else s for y, s in zip(yard, fallback or (0.0, 0.0)))
    ratio = tuple(e / u if u > 0.0 else (0.0 if e == 0.0 else float("inf")) for e, u in zip(err, used))
    res = dict(label=label, method=method, native=dict(native_stats), replay=dict(r64.stats), yardstick=yard, yardstick_used=used,
               error=err, ratio=ratio, margin=min(threshold_margin(r32), threshold_margin(r64)),
               same_sequence=all(decisions(r) == decisions(r64) and all(r.stats[k] == r64.stats[k] for k in ("nfe", "steps", "rejects"))
                                 for r in (r32, *nudges, *moved)),
               spread=max((_err(r.out.detach().cpu(), o64) for r in moved), default=0.0))
    st = {k: r64.stats[k] for k in ("nfe", "steps", "rejects")}
    line = (f"{label or method:<34} {method:<14} replay nfe {st['nfe']:>5} steps {st['steps']:>4} rejects {st['rejects']:>2} | native nfe "
            f"{native_stats['nfe']:>5} steps {native_stats['steps']:>4} rejects {native_stats['rejects']:>2} | margin {res['margin']:.2e} spread {res['spread']:.2e} | "
            f"valid: yardstick {yard[0]:.3e} native {err[0]:.3e} ratio {ratio[0]:.2f} | whole: yardstick {yard[1]:.3e} native {err[1]:.3e} "
            f"ratio {ratio[1]:.2f}" + ("" if used == yard else f" (family yardstick {used[0]:.3e} / {used[1]:.3e})"))
    print(line)
    path = os.environ.get("ODE_REPLAY_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")
    assert torch.isfinite(out).all()
    # 1. the decision sequence is a property of the problem
    assert res["same_sequence"], ("the replays decide differently: choose another seed", r64.stats, r32.stats, [r.stats for r in (*nudges, *moved)])
    if margin:
        assert res["margin"] >= MARGIN, ("a decision value lies within the margin of its threshold: choose another seed", res["margin"])
    assert res["spread"] <= FACTOR * used[1], ("one fp32 ulp of z moves the float64-state replay by more than the gate allows the "
                                               "native solve: choose another seed", res["spread"], used[1])
    # 2. the native controller takes that sequence
    if check_stats:
        assert {k: native_stats[k] for k in st} == st, (dict(native_stats), st)
    # 3. the native result is as close to the float64 replay as fp32 is
    assert err[0] <= FACTOR * used[0] and err[1] <= FACTOR * used[1], (err, used)
    return res
