"""Native feature front end against the reference computation on the same GPU (F.pad + torch.stft through the ROCm FFT library
+ magnitude + matmul + log, utils/audio.py:19-26,50-52), both warmed up, device-synchronised timing with HIP events.

    python tools/mel_bench.py [--reps 20] [--warmup 5] [--json out.json]

Shapes: B = 1 x 5 s (api.py's reference clip), B = 64 x 10 s padded, 256 ragged utterances of 1-15 s (preprocessing; native:
one ragged launch, reference: one call per utterance), and the seven multi-scale configs of vocoders/vocos/models/loss.py at
B = 16 x 2 s.  Reports frames per second and the HBM bound from the bytes the shapes imply (fp32 samples read once, output
written once) at the MI355X's 8 TB/s peak.  Kernel times come from a separate rocprofv3 --kernel-trace --stats run.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8.0e12
SR = 44100


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _reference(m):
    """utils/audio.py's forward on the module's own buffers, in torch."""
    win, fb = m.spectrogram.window, m.mel_scale.fb

    def run(w):
        x = F.pad(w.unsqueeze(1), (m.pad, m.pad), "reflect").squeeze(1)
        spec = torch.view_as_real(torch.stft(x, m.n_fft, m.hop_length, m.win_length, win, False, "reflect", False, True, True))
        spec = torch.sqrt(spec.pow(2).sum(-1) + 1e-6)
        return torch.log(torch.clamp(torch.matmul(spec.transpose(-1, -2), fb).transpose(-1, -2), min=1e-5))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--native-only", action="store_true", help="skip the torch reference (profiling runs)")
    args = ap.parse_args()
    from stabletts_amd.audio import LogMelSpectrogram
    torch.manual_seed(0)
    rows = []

    def mod(n_fft=2048, n_mels=128):
        hop = n_fft // 4
        return LogMelSpectrogram(SR, n_fft, n_fft, hop, 0.0, None, (n_fft - hop) // 2, n_mels, False, "reflect", "slaney").cuda()

    def report(name, m, native, ref, n_frames, n_samples, n_out):
        t_nat = _time(native, args.reps, args.warmup)
        t_ref = _time(ref, args.reps, args.warmup) if ref is not None else float("nan")
        bound_us = (4 * n_samples + 4 * n_out) / HBM * 1e6
        r = dict(shape=name, n_fft=m.n_fft, n_mels=m.n_mels, frames=n_frames, native_ms=round(t_nat, 4), reference_ms=round(t_ref, 4),
                 speedup=round(t_ref / t_nat, 2) if ref is not None else None, native_mframes_per_s=round(n_frames / t_nat / 1e3, 2),
                 hbm_bound_us=round(bound_us, 2), native_vs_bound=round(t_nat * 1e3 / bound_us, 1))
        print(json.dumps(r), flush=True)
        rows.append(r)

    with torch.inference_mode():
        for name, B, secs in (("B=1 x 5 s", 1, 5.0), ("B=64 x 10 s", 64, 10.0)):
            m = mod()
            w = 0.1 * torch.randn(B, int(secs * SR), device="cuda")
            T = m.frames(w.shape[1])
            ref = _reference(m)
            report(name, m, lambda: m(w), None if args.native_only else (lambda: ref(w)), B * T, w.numel(), B * m.n_mels * T)
        m = mod()
        rng = np.random.Generator(np.random.PCG64(1))
        lens = rng.integers(1 * SR, 15 * SR, size=256)
        waves = [0.1 * torch.randn(int(n), device="cuda") for n in lens]
        T = sum(m.frames(int(n)) for n in lens)
        ref = _reference(m)
        report("256 ragged x 1-15 s", m, lambda: m.forward_ragged(waves),
               None if args.native_only else (lambda: [ref(x[None]) for x in waves]), T, int(lens.sum()), m.n_mels * T)
        for n_mels, n_fft in zip([5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048]):
            m = mod(n_fft, n_mels)
            w = 0.1 * torch.randn(16, 2 * SR, device="cuda")
            T = m.frames(w.shape[1])
            ref = _reference(m)
            report(f"B=16 x 2 s, n_fft {n_fft}", m, lambda: m(w), None if args.native_only else (lambda: ref(w)), 16 * T, w.numel(),
                   16 * n_mels * T)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
