"""Checks of the split-precision FireflyGAN vocoder ("f16_split" / "bf16_split": every MFMA operand a hi + lo pair of the 16-bit
format, w_hi x_hi + w_hi x_lo + w_lo x_hi in fp32), shared by test_ffgan_split_cpu.py and test_gpu_ffgan_split.py.

The emulation is the float64 restatement (tests/ffgan_restatement.py) with ``R.rounder`` wrapped: a split name rounds a value to
hi + lo, hi = fl16(x), lo = fl16(x - hi), x the fp32 value (fp32 first, as on the device).  The dropped lo * lo product (2^-22 per
product for f16) is NOT emulated: it falls inside the gate's fp32 allowance.

Accuracy gate, per compared tensor, e = max |. - float64| / max |float64|:
    e_native <= e_emul_split + 4 * e_fp32      and      e_native < 1e-3
e_emul_split: the restatement with split-rounded weights and inputs; e_fp32: the same restatement code run in float32 on the CPU.
The factor 4 is the project's standing allowance for an fp32 device path against torch fp32's own distance from float64.
"""
import contextlib
import functools

import torch

from tests import ffgan_restatement as R
from tests.ffgan_checks import CONFIGS, NAMES, build, run_captured

SPLIT = {"f16_split": torch.float16, "bf16_split": torch.bfloat16}
BAR = 1e-3

_plain_rounder = R.rounder


def split_pair(t, td):
    """-> (hi, lo) as float32: hi = fl16(x), lo = fl16(x - hi) of the fp32 value x."""
    x = t.to(torch.float32)
    hi = x.to(td).to(torch.float32)
    lo = (x - hi).to(td).to(torch.float32)      # x - hi is exact in fp32
    return hi, lo


def rounder(dtype):
    """R.rounder plus the two split names: x -> hi + lo (exact in float64)."""
    if dtype not in SPLIT:
        return _plain_rounder(dtype)
    td = SPLIT[dtype]

    def f(t):
        hi, lo = split_pair(t, td)
        return (hi.double() + lo.double()).to(t.dtype)
    return f


@contextlib.contextmanager
def _split_names():
    """R.prepare / R.forward look ``rounder`` up in their module: the wrapper stands in for the duration of one call."""
    R.rounder = rounder
    try:
        yield
    finally:
        R.rounder = _plain_rounder


def forward_emulated(sd, cfg, mel, dt):
    with _split_names():
        return R.forward(sd, cfg, mel, dt, dt)


def forward_fp32(sd, cfg, mel):
    return R.forward(sd, cfg, mel, prepared=R.prepare(sd, None, dtype=torch.float32))


def errors(out, ref, names=NAMES):
    return {n: R.rel_max(out[n], ref[n]) for n in names}


def gate(tag, got, ref, e_emul, e_fp32, names=NAMES):
    """Prints every pair; -> the largest e_native / (e_emul_split + 4 e_fp32)."""
    bad, worst = [], 0.0
    for name in names:
        assert tuple(got[name].shape) == tuple(ref[name].shape), (name, got[name].shape, ref[name].shape)
        assert bool(torch.isfinite(got[name]).all()), name
        e_native = R.rel_max(got[name], ref[name])
        bound = e_emul[name] + 4 * e_fp32[name]
        worst = max(worst, e_native / bound)
        print(f"ffgan_split_parity {tag:<30} {name:<9} e_native {e_native:.3e}   e_emul_split {e_emul[name]:.3e}   e_fp32 {e_fp32[name]:.3e}   "
              f"ratio {e_native / bound:.3f}")
        if not (e_native <= bound and e_native < BAR):
            bad.append((name, e_native, bound))
    assert not bad, bad
    return worst


_models = {}


def model(name, dt):
    """The native module of CONFIGS[name] ("default": R.DEFAULT), kept for the session: the tests share them."""
    if (name, dt) not in _models:
        _models[(name, dt)] = build(R.DEFAULT if name == "default" else CONFIGS[name], dt)[0]
    return _models[(name, dt)]


@functools.lru_cache(maxsize=None)
def _cpu_side(name, B, T, mel_seed):
    """State dict, mel, float64 restatement and its float32 run: made once per case, shared by the dtypes, never written to."""
    cfg = R.DEFAULT if name == "default" else CONFIGS[name]
    sd = R.make_state_dict(cfg, R.SEED)
    mel = R.make_mel(B, T, cfg["backbone"]["input_channels"], mel_seed)
    ref = R.forward(sd, cfg, mel)
    return cfg, sd, mel, ref, errors(forward_fp32(sd, cfg, mel), ref)


@functools.lru_cache(maxsize=None)
def _emulated(name, B, T, mel_seed, dt):
    cfg, sd, mel, ref, _ = _cpu_side(name, B, T, mel_seed)
    return errors(forward_emulated(sd, cfg, mel, dt), ref)


def against_restatement(name, dt, B, T, mel_seed, ref=None):
    """The split-precision native module on make_mel(B, T, ., mel_seed) against float64 (`ref`: another float64 reference of the
    same case, e.g. the real module's fixture) under the gate above; -> (the worst ratio, e_native of the audio)."""
    _, _, mel, ref64, e_fp32 = _cpu_side(name, B, T, mel_seed)
    got = run_captured(model(name, dt), mel)
    ref = ref64 if ref is None else ref
    worst = gate(f"{name} {B}x{T} {dt}", got, ref, _emulated(name, B, T, mel_seed, dt), e_fp32)
    return worst, R.rel_max(got["audio"], ref["audio"])
