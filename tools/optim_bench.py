"""Times the optimizer part of a training step natively (stabletts_amd.optim: clip_grad_norm_ + AdamW.step) against torch on the
same GPU, on the real parameter shapes of the two training loops with synthetic gradients (no model runs):

  vocos_step   vocoders/vocos/train.py: clip_grad_norm_(., 1000) on the MPD, the MRD and the generator (:108-109,130), then
               AdamW.step() of optimizer_d (MPD + MRD) and optimizer_g (generator) (:73-74)
  tts_step     train.py:60: one AdamW.step() over StableTTS(401, 128, 256, 1024, 4, 3, 6, 3, 0.1, 256) (BASELINE config 2's model);
               train.py does not clip

Three sides on copies of the same parameters and gradients: native, torch's clip_grad_norm_ with AdamW() (default foreach) and
with AdamW(fused=True).  The sides run interleaved after a warm-up; prints one JSON line per workload with the medians in ms per
step (host and device: what a training loop waits for), the device launches of one step of each side and the time the device
was busy in them (torch.profiler: kernels, fills and copies), and the achieved GB/s of the native side against 28 bytes per
parameter (the update reads p, g, m, v and writes p, m, v; the norm's read pass is not counted), per step and per busy time.

    python tools/optim_bench.py [--steps 20] [--warmup 3]      (recorded in profiles/optim_bench.txt)
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _launches(f):
    from torch.profiler import ProfilerActivity, profile
    f()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        f()
        torch.cuda.synchronize()
    rows = prof.key_averages()
    busy_us = sum(getattr(r, "self_device_time_total", None) or getattr(r, "self_cuda_time_total", 0) for r in rows)
    return sum(r.count for r in rows), busy_us / 1e3


def _shapes(module):
    return [tuple(p.shape) for p in module.parameters()]


def _vocos_lists():
    import types

    from oracle import vocos_oracle as vo
    from stabletts_amd.discriminator import MultiPeriodDiscriminator, MultiResolutionDiscriminator
    from stabletts_amd.vocos_train import Vocos
    c = vo.VocosConfig
    gen = Vocos(types.SimpleNamespace(input_channels=c.input_channels, dim=c.dim, intermediate_dim=c.intermediate_dim, num_layers=c.num_layers),
                types.SimpleNamespace(n_fft=c.n_fft, hop_length=c.hop_length))
    return {"mpd": _shapes(MultiPeriodDiscriminator()), "mrd": _shapes(MultiResolutionDiscriminator()), "generator": _shapes(gen)}


def _tts_lists():
    from stabletts_amd.model import StableTTS
    return {"model": _shapes(StableTTS(401, 128, 256, 1024, 4, 3, 6, 3, 0.1, 256))}


class _Side:
    """One side's copy of the workload: parameters with gradients, its optimizers and its clip function."""

    def __init__(self, lists, optimizers, clips, make_opt, clip):
        gen = torch.Generator(device="cuda").manual_seed(3)
        self.params = {k: [torch.randn(s, device="cuda", generator=gen).requires_grad_(True) for s in shapes] for k, shapes in lists.items()}
        for ps in self.params.values():
            for p in ps:
                p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
        self.opts = [make_opt([p for k in keys for p in self.params[k]]) for keys in optimizers]
        self.clips, self.clip = clips, clip

    def step(self):
        for k in self.clips:
            self.clip(self.params[k], 1000)
        for o in self.opts:
            o.step()


def _workload(name, lists, optimizers, clips, warmup, steps):
    from stabletts_amd import optim
    sides = {"native": _Side(lists, optimizers, clips, lambda ps: optim.AdamW(ps, lr=1e-4), optim.clip_grad_norm_),
             "torch_foreach": _Side(lists, optimizers, clips, lambda ps: torch.optim.AdamW(ps, lr=1e-4), torch.nn.utils.clip_grad_norm_),
             "torch_fused": _Side(lists, optimizers, clips, lambda ps: torch.optim.AdamW(ps, lr=1e-4, fused=True), torch.nn.utils.clip_grad_norm_)}
    assert all(o._native_device() is not None for o in sides["native"].opts)
    for _ in range(warmup):
        for s in sides.values():
            _timed(s.step)
    times = {k: [] for k in sides}
    for _ in range(steps):
        for k, s in sides.items():
            times[k].append(_timed(s.step))
    n_params = sum(p.numel() for ps in sides["native"].params.values() for p in ps)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"workload": name, "tensors": sum(len(v) for v in lists.values()), "parameters": n_params, "clips_per_step": len(clips),
           "optimizers": len(optimizers), "steps": steps}
    for k in sides:
        out[k + "_ms_median"] = round(med[k], 4)
    for k in ("torch_foreach", "torch_fused"):
        out[k + "_over_native_median"] = round(statistics.median([y / x for x, y in zip(times["native"], times[k])]), 3)
    for k, s in sides.items():
        out[k + "_launches"], busy = _launches(s.step)
        out[k + "_device_busy_ms"] = round(busy, 4)
    out["native_gbytes_per_s_at_28B"] = round(28 * n_params / (med["native"] * 1e-3) / 1e9, 1)
    out["native_gbytes_per_s_at_28B_device_busy"] = round(28 * n_params / (out["native_device_busy_ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    _workload("vocos_step", _vocos_lists(), [("mpd", "mrd"), ("generator",)], ["mpd", "mrd", "generator"], a.warmup, a.steps)
    _workload("tts_step", _tts_lists(), [("model",)], [], a.warmup, a.steps)


if __name__ == "__main__":
    main()
