"""Times one training step (forward + backward of a seeded projection loss) of the MelStyleEncoder and of the
DurationPredictor natively (native_training, st_*_train_forward / _backward) against torch autograd through the torch
restatement of the two modules (tests/style_dp_restatement.py) on the same GPU, at train.py's shapes: reference slices of
T in {100, 333} frames (random_slice_tensor takes length/12 .. length/3 of <= 1000 frames), token lengths up to 200, ragged
(lengths 60-100 % of T).  Dropout on in both legs (train mode, the reference's p).  The legs are paired and interleaved
after a warm-up; prints one JSON line per (module, B, T) with the medians and the per-pair ratio torch / native.

    python tools/style_dp_train_bench.py [--B 32 64] [--steps 30]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--B", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import style_dp_restatement as R
    import synth_weights as sw
    from stabletts_amd.duration_predictor_train import DurationPredictor
    from stabletts_amd.reference_encoder_train import MelStyleEncoder
    style = MelStyleEncoder(sw.N_MELS, style_vector_dim=sw.GIN, style_kernel_size=5, dropout=0.25)
    style.load_state_dict(sw.style_encoder_state_dict())
    style = style.cuda().train()
    dp = DurationPredictor(sw.DP_HIDDEN, sw.DP_FILTER, sw.DP_KERNEL, 0.5, sw.GIN)
    dp.load_state_dict(sw.duration_predictor_state_dict())
    dp = dp.cuda().train()
    ssd = {k: v.cuda().requires_grad_(True) for k, v in sw.style_encoder_state_dict().items()}
    dsd = {k: v.cuda().requires_grad_(True) for k, v in sw.duration_predictor_state_dict().items()}
    drop_t = torch.nn.functional.dropout
    for B in a.B:
        rng = np.random.Generator(np.random.PCG64(B))
        for T in (100, 333):
            lengths = [T] + [int(v) for v in rng.integers(int(0.6 * T), T + 1, size=B - 1)]
            y, m = sw.style_inputs(B, T, lengths, 3)
            y, m = torch.from_numpy(y).cuda(), torch.from_numpy(m).cuda()
            w = torch.randn(B, sw.GIN, device="cuda")

            def nat():
                (style(y, m) * w).sum().backward()

            def ref():      # torch's own dropout on the restatement's sites (same p, its own masks)
                ones = {k: drop_t(torch.ones(B, sw.STYLE_HIDDEN, T, device="cuda"), 0.25) for k in ("spec0", "spec1", "glu0", "glu1")}
                ones["attn"] = drop_t(torch.ones(B, 2, T, T, device="cuda"), 0.25)
                (R.style_forward(ssd, y, m, drop=ones) * w).sum().backward()

            print(json.dumps({"workload": "style_encoder_train_step", "B": B, "T": T, "steps": a.steps, **_pair(nat, ref, a.warmup, a.steps)}))
        Tx = 200
        lengths = [Tx] + [int(v) for v in rng.integers(int(0.6 * Tx), Tx + 1, size=B - 1)]
        x, xm, g = (torch.from_numpy(t).cuda() for t in sw.dp_inputs(B, Tx, lengths, 4))
        wl = torch.randn(B, 1, Tx, device="cuda")

        def nat_dp():
            (dp(x, xm, g) * wl).sum().backward()

        def ref_dp():
            ones = {k: drop_t(torch.ones(B, sw.DP_FILTER, Tx, device="cuda"), 0.5) for k in ("norm1", "norm2")}
            (R.dp_forward(dsd, x, xm, g, drop=ones) * wl).sum().backward()

        print(json.dumps({"workload": "duration_predictor_train_step", "B": B, "Tx": Tx, "steps": a.steps, **_pair(nat_dp, ref_dp, a.warmup, a.steps)}))


if __name__ == "__main__":
    main()
