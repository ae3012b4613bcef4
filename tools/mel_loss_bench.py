"""The Vocos multi-scale mel loss step (vocoders/vocos/train.py:115, models/loss.py): seven log-mel scales (n_fft 32 ... 2048) on the
generator's output x and the target y, the L1 sum and the backward to x -- native (stabletts_amd.audio_train: st_mel_forward +
st_mel_backward) against the same computation in torch on the same GPU (tools/mel_bench.py's reference: F.pad + torch.stft +
magnitude + matmul + log, with autograd).  Both warmed up and alternated in one process; each repeat times --steps loss steps with
HIP events.

    python tools/mel_loss_bench.py [--batch 32] [--samples 20480] [--steps 20] [--repeats 7] [--warmup 5] [--native-only]

The default shape is the trainer's (TrainConfig: batch 32 x segment 20480 samples).  --native-only skips the torch side, for a
separate rocprofv3 --kernel-trace --stats run.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SCALES = list(zip([5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048]))      # loss.py:11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=20480)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--native-only", action="store_true", help="skip the torch side (profiling runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from mel_bench import _reference
    from stabletts_amd.audio_train import LogMelSpectrogram
    mods = [LogMelSpectrogram(44100, n, n, n // 4, 0.0, None, (n - n // 4) // 2, m, False, "reflect", "slaney").cuda() for m, n in SCALES]
    refs = [_reference(m) for m in mods]
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (0.3 * torch.randn(args.batch, 1, args.samples, device="cuda", generator=g)).requires_grad_(True)
    y = 0.3 * torch.randn(args.batch, 1, args.samples, device="cuda", generator=g)

    def native():
        loss = sum(F.l1_loss(m(x), m(y)) for m in mods)
        loss.backward()
        return loss

    def reference():
        loss = sum(F.l1_loss(r(x.squeeze(1)), r(y.squeeze(1))) for r in refs)
        loss.backward()
        return loss

    sides = [("native", native)] + ([] if args.native_only else [("torch", reference)])
    for _, fn in sides:
        for _ in range(args.warmup):
            x.grad = None
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in sides}
    for _ in range(args.repeats):
        for name, fn in sides:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                x.grad = None
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / args.steps)
    r = dict(shape=f"B={args.batch} x {args.samples}", scales=[n for _, n in SCALES], steps=args.steps, repeats=args.repeats)
    for name, ts in times.items():
        r[name + "_ms"] = round(statistics.median(ts), 4)
        r[name + "_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    if not args.native_only:
        r["speedup"] = round(r["torch_ms"] / r["native_ms"], 2)
        x.grad = None
        ln = native()
        dn = x.grad.clone()
        x.grad = None
        lt = reference()
        r["loss_rel_diff"] = float(abs(ln.detach() - lt.detach()) / lt.detach().abs())
        r["grad_cosine"] = float(F.cosine_similarity(dn.flatten(), x.grad.flatten(), dim=0))
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
