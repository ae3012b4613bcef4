"""Times the Vocos generator's forward + backward natively (stabletts_amd.vocos_train: st_vocos_train_forward / _backward, fp32)
against torch autograd through the same forward written in torch ops (tests/vocos_vjp_restatement.torch_vocos, fp32) on the same
GPU, at the shape of vocoders/vocos/train.py (batch_size 32 x segment_size 20480 -> B = 32, T = 40) and at B = 16, T = 200.
Two losses per shape: a seeded projection sum(audio * W) (the generator alone), and the mel-loss-only generator step of
train.py:94,115,128 -- forward, the seven-scale log-mel L1 loss (native spectrograms, stabletts_amd.audio_train, in both legs) and
backward.  The legs are paired and interleaved after a warm-up; prints one JSON line per (workload, B, T) with the medians and
the per-pair ratio torch / native, and, with --kernels, the native leg's largest kernels (torch.profiler).

    python tools/vocos_train_bench.py [--steps 30] [--kernels] [--dim D] [--intermediate-dim F] [--num-layers L]

The default generator is the inference preset (512 / 1536 / 8); --dim 768 --intermediate-dim 2048 --num-layers 12 is the one the
reference's trainer builds (vocoders/vocos/config.py:21-26).
"""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCALES = list(zip([5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048]))      # loss.py:11


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--dim", type=int)
    ap.add_argument("--intermediate-dim", type=int)
    ap.add_argument("--num-layers", type=int)
    a = ap.parse_args()
    from oracle import vocos_oracle as vo
    from stabletts_amd.audio_train import LogMelSpectrogram
    from stabletts_amd.vocos_train import Vocos
    from tests import vocos_vjp_restatement as R
    c = vo.vocos_config(**{k: v for k, v in (("dim", a.dim), ("intermediate_dim", a.intermediate_dim), ("num_layers", a.num_layers)) if v})
    sd = vo.make_vocos_state_dict(7, c)
    gen = {"dim": c.dim, "intermediate_dim": c.intermediate_dim, "num_layers": c.num_layers}
    voc = Vocos(types.SimpleNamespace(input_channels=c.input_channels, dim=c.dim, intermediate_dim=c.intermediate_dim, num_layers=c.num_layers),
                types.SimpleNamespace(n_fft=c.n_fft, hop_length=c.hop_length))
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    voc = voc.cuda().train()
    tp = {k: torch.from_numpy(v).cuda().requires_grad_(k != "head.istft.window") for k, v in sd.items()}
    mods = [LogMelSpectrogram(44100, n, n, n // 4, 0.0, None, (n - n // 4) // 2, m, False, "reflect", "slaney").cuda() for m, n in SCALES]
    mel_loss = lambda y, x: sum(F.l1_loss(m(y), m(x)) for m in mods)      # noqa: E731
    for B, T in ((32, 40), (16, 200)):
        mel = torch.from_numpy(vo.make_mel(B, T, 3)).cuda()
        W = torch.randn(B, T * c.hop_length, device="cuda")
        y = 0.1 * torch.randn(B, 1, T * c.hop_length, device="cuda")

        def zero():
            for p in voc.parameters():
                p.grad = None
            for p in tp.values():
                p.grad = None

        def nat():
            zero(); (voc(mel) * W).sum().backward()

        def ref():
            zero(); (R.torch_vocos(tp, mel, c.num_layers) * W).sum().backward()

        def nat_step():
            zero(); mel_loss(y, voc(mel).unsqueeze(1)).backward()

        def ref_step():
            zero(); mel_loss(y, R.torch_vocos(tp, mel, c.num_layers).unsqueeze(1)).backward()

        print(json.dumps({"workload": "vocos_forward_backward", **gen, "B": B, "T": T, "steps": a.steps, **_pair(nat, ref, a.warmup, a.steps)}), flush=True)
        print(json.dumps({"workload": "vocos_mel_loss_generator_step", **gen, "B": B, "T": T, "steps": a.steps,
                          **_pair(nat_step, ref_step, a.warmup, a.steps)}), flush=True)
        if a.kernels:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(5):
                    nat()
                torch.cuda.synchronize()
            rows = sorted(prof.key_averages(), key=lambda r: -r.device_time_total)[:8]
            tot = sum(r.device_time_total for r in prof.key_averages())
            for r in rows:
                print(json.dumps({"kernel": r.key[:90], "B": B, "T": T, "share": round(r.device_time_total / tot, 3),
                                  "us_per_step": round(r.device_time_total / 5, 1), "calls_per_step": r.count // 5}), flush=True)


if __name__ == "__main__":
    main()
