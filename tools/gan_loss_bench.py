"""Times the three scalar GAN losses of a Vocos training step natively (stabletts_amd.gan_loss) against the torch expressions of
vocoders/vocos/models/loss.py:37-66 on the same GPU, at the shape of vocoders/vocos/train.py (batch_size 32 x segment_size 20480:
64 signals).  No discriminator runs: the feature maps are random fp32 leaves (requires_grad) of the shapes the native
discriminators report (period_disc_fmap_shapes for periods 2, 3, 5, 7, 11; resolution_disc_fmap_shapes for windows 2048, 1024,
512), and both sides get each map's halves f[:B], f[B:], as the native discriminators return them.

  discriminator_leg   discriminator_loss on the period and the resolution logits, backward to the maps
  generator_leg       feature_loss + generator_loss for both discriminators, backward to the maps

Forward plus backward, the two sides interleaved after a warm-up; prints one JSON line per leg with the medians, the per-pair
ratio torch / native, and the device launches of one iteration of each side (torch.profiler: kernels, fills and copies).

    python tools/gan_loss_bench.py [--steps 10] [--B 32] [--T 20480]      (recorded in profiles/gan_loss_bench.txt)
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
    return sum(r.count for r in prof.key_averages())


def _pair(native, torch_leg, warmup, steps):
    for _ in range(warmup):
        _timed(native); _timed(torch_leg)
    tn, tt = [], []
    for _ in range(steps):
        tn.append(_timed(native)); tt.append(_timed(torch_leg))
    return {"native_ms_median": round(statistics.median(tn), 3), "torch_fp32_ms_median": round(statistics.median(tt), 3),
            "torch_over_native_median": round(statistics.median([y / x for x, y in zip(tn, tt)]), 3),
            "native_launches": _launches(native), "torch_launches": _launches(torch_leg)}


def _torch_feature(fr, fg):
    return 2 * sum(torch.mean(torch.abs(rl - gl)) for dr, dg in zip(fr, fg) for rl, gl in zip(dr, dg))


def _torch_disc(rs, gs):
    loss, r_losses, g_losses = 0, [], []
    for dr, dg in zip(rs, gs):
        r_loss, g_loss = torch.mean((1 - dr) ** 2), torch.mean(dg ** 2)
        loss = loss + (r_loss + g_loss)
        r_losses.append(r_loss.item()); g_losses.append(g_loss.item())         # the reference's two host reads per discriminator
    return loss


def _torch_gen(gs):
    return sum(torch.mean((1 - dg) ** 2) for dg in gs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=20480)
    a = ap.parse_args()
    from stabletts_amd import _lib, gan_loss
    from stabletts_amd.discriminator import DiscriminatorR
    B, T = a.B, a.T
    gen = torch.Generator(device="cuda").manual_seed(11)
    groups = []                                     # per discriminator: its maps, the last one the logits
    for p in (2, 3, 5, 7, 11):
        eng = _lib.Engine(0, 0, 0, 0, 0, 0, 0, "f16", 0, period_discriminator=dict(period=p, lrelu_slope=0.1))
        groups.append(("period", eng.period_disc_fmap_shapes(2 * B, T, p)))
        eng.close()
    for W in (2048, 1024, 512):
        eng = DiscriminatorR(W).cuda().engine()
        groups.append(("resolution", eng.resolution_disc_fmap_shapes(2 * B, T)))
    maps = [[torch.randn(s, device="cuda", generator=gen).requires_grad_(True) for s in shapes] for _, shapes in groups]
    leaves = [f for d in maps for f in d]
    fr, fg = [[f[:B] for f in d] for d in maps], [[f[B:] for f in d] for d in maps]
    rs, gs = [d[-1] for d in fr], [d[-1] for d in fg]

    def zero():
        for f in leaves:
            f.grad = None

    def nat_disc():
        zero(); gan_loss.discriminator_loss(rs, gs)[0].backward()

    def ref_disc():
        zero(); _torch_disc(rs, gs).backward()

    def nat_gen():
        zero(); (gan_loss.feature_loss(fr, fg) + gan_loss.generator_loss(gs)[0]).backward()

    def ref_gen():
        zero(); (_torch_feature(fr, fg) + _torch_gen(gs)).backward()

    head = {"B": B, "T": T, "signals": 2 * B, "steps": a.steps,
            "period_pairs": sum(len(s) for k, s in groups if k == "period"), "resolution_pairs": sum(len(s) for k, s in groups if k == "resolution"),
            "map_gbytes": round(sum(f.numel() for f in leaves) * 4 / 1e9, 3)}
    print(json.dumps({"workload": "discriminator_leg", **head, **_pair(nat_disc, ref_disc, a.warmup, a.steps)}), flush=True)
    print(json.dumps({"workload": "generator_leg", **head, **_pair(nat_gen, ref_gen, a.warmup, a.steps)}), flush=True)


if __name__ == "__main__":
    main()
