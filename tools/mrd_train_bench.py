"""Times the multi-resolution discriminator's two legs of a Vocos training step natively (stabletts_amd.discriminator, fp32)
against torch autograd through the same module written in torch ops (tests/mrd_restatement.mrd_forward, fp32; its spectrum is a
DFT matrix product, which the GPU runs as a GEMM) on the same GPU, at the shape of vocoders/vocos/train.py (batch_size 32 x
segment_size 20480: 64 signals through the three resolutions):

  discriminator_leg          train.py:102-106: mrd(y, y_hat.detach()), discriminator_loss, backward to the parameters only
  generator_leg              train.py:123-128: mrd(y, y_hat), feature_loss + generator_loss, backward to y_hat and the parameters
  generator_leg_frozen       the same with the module's parameters frozen (requires_grad_(False)): backward to y_hat only

The legs are paired and interleaved after a warm-up; prints one JSON line per workload with the medians and the per-pair ratio
torch / native, and, with --kernels, the native legs' largest kernels (torch.profiler).  The torch side's losses use no sign
bookkeeping (torch.abs; mrd_restatement's where-form of the leaky ReLU costs it one extra elementwise op per layer).

    python tools/mrd_train_bench.py [--steps 10] [--B 32] [--T 20480] [--kernels]      (recorded in profiles/mrd_train_bench.txt)
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


def _pair(native, torch_leg, warmup, steps):
    for _ in range(warmup):
        _timed(native); _timed(torch_leg)
    tn, tt = [], []
    for _ in range(steps):
        tn.append(_timed(native)); tt.append(_timed(torch_leg))
    return {"native_ms_median": round(statistics.median(tn), 3), "torch_fp32_ms_median": round(statistics.median(tt), 3),
            "torch_over_native_median": round(statistics.median([y / x for x, y in zip(tn, tt)]), 3)}


def _disc_loss(rs, gs):
    return sum(torch.mean((1 - dr) ** 2) + torch.mean(dg ** 2) for dr, dg in zip(rs, gs))


def _gen_loss(gs, fr, fg):
    feat = 2 * sum(torch.mean(torch.abs(rl - gl)) for dr, dg in zip(fr, fg) for rl, gl in zip(dr, dg))
    return feat + sum(torch.mean((1 - dg) ** 2) for dg in gs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=20480)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    from stabletts_amd.discriminator import MultiResolutionDiscriminator
    from tests import mrd_restatement as R
    B, T = a.B, a.T
    sd_np = R.make_mrd_state_dict(7)
    mrd = MultiResolutionDiscriminator()
    mrd.load_state_dict({k: torch.from_numpy(v) for k, v in R.with_windows(sd_np).items()}, strict=True)
    mrd = mrd.cuda().train()
    tp = R.to_torch(sd_np, dtype=torch.float32, device="cuda", requires_grad=True)
    y = torch.from_numpy(R.make_audio(B, T, 8)).cuda()
    y_hat = torch.from_numpy(R.make_audio(B, T, 9)).cuda()

    def torch_mrd(fake):
        outs = R.mrd_forward(tp, y, fake)
        lg = [o.fmaps[-1] for o in outs]
        return [l[:B] for l in lg], [l[B:] for l in lg], [[f[:B] for f in o.fmaps] for o in outs], [[f[B:] for f in o.fmaps] for o in outs]

    def zero():
        for p in list(mrd.parameters()) + list(tp.values()):
            p.grad = None

    def freeze(flag):
        mrd.requires_grad_(not flag)
        for p in tp.values():
            p.requires_grad_(not flag)

    def nat_disc():
        zero(); rs, gs, _, _ = mrd(y, y_hat.detach()); _disc_loss(rs, gs).backward()

    def ref_disc():
        zero(); rs, gs, _, _ = torch_mrd(y_hat.detach()); _disc_loss(rs, gs).backward()

    def nat_gen():
        zero(); f = y_hat.clone().requires_grad_(True); _, gs, fr, fg = mrd(y, f); _gen_loss(gs, fr, fg).backward()

    def ref_gen():
        zero(); f = y_hat.clone().requires_grad_(True); _, gs, fr, fg = torch_mrd(f); _gen_loss(gs, fr, fg).backward()

    head = {"B": B, "T": T, "signals": 2 * B, "steps": a.steps}
    print(json.dumps({"workload": "discriminator_leg", **head, **_pair(nat_disc, ref_disc, a.warmup, a.steps)}), flush=True)
    print(json.dumps({"workload": "generator_leg", **head, **_pair(nat_gen, ref_gen, a.warmup, a.steps)}), flush=True)
    freeze(True)
    print(json.dumps({"workload": "generator_leg_frozen", **head, **_pair(nat_gen, ref_gen, a.warmup, a.steps)}), flush=True)
    freeze(False)
    if a.kernels:
        from torch.profiler import ProfilerActivity, profile
        for name, leg in (("discriminator_leg", nat_disc), ("generator_leg", nat_gen)):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(2):
                    leg()
                torch.cuda.synchronize()
            tot = sum(r.device_time_total for r in prof.key_averages())
            for r in sorted(prof.key_averages(), key=lambda r: -r.device_time_total)[:8]:
                print(json.dumps({"leg": name, "kernel": r.key[:90], "share": round(r.device_time_total / tot, 3),
                                  "ms_per_step": round(r.device_time_total / 2e3, 3), "calls_per_step": r.count // 2}), flush=True)


if __name__ == "__main__":
    main()
