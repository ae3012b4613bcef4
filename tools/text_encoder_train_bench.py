"""Times one training step of the TextEncoder (forward + backward of loss = sum(mu_x * W)) natively against torch autograd
through the fp32 oracle restatement (oracle.text_encoder_forward) on the same GPU, at B=64 x T=300 ragged (lengths 60-100 % of
T), dropout off in both legs (eval mode).  The two legs are paired and interleaved (native, torch, native, ...) after a warm-up; prints the median of each and the
per-pair ratio as one JSON line.

    python tools/text_encoder_train_bench.py [--steps 30] [--dt f16]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dt", default="f16")
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=300)
    a = ap.parse_args()
    import oracle
    from oracle.make_golden_text_encoder import text_inputs
    from stabletts_amd.text_encoder import TextEncoder
    sd = oracle.make_text_encoder_state_dict(2468)
    rng = np.random.Generator(np.random.PCG64(1))
    lengths = [a.T] + [int(v) for v in rng.integers(int(0.6 * a.T), a.T + 1, size=a.B - 1)]
    tok, c, lens = text_inputs(a.B, a.T, lengths, 7)
    tok, c, lens = tok.cuda(), c.cuda(), lens.cuda()
    w = torch.randn(a.B, 128, a.T, device="cuda")
    m = TextEncoder(401, 128, 256, 1024, 4, 3, 3, 0.1, 256, operand_dtype=a.dt)
    m.load_state_dict(sd)
    m = m.cuda().eval()      # dropout off, as in the torch leg: both legs do the same work
    pr = {k: v.cuda().requires_grad_(True) for k, v in sd.items()}

    def native():
        cc = c.clone().requires_grad_(True)
        _, mu_x, _ = m(tok, cc, lens)
        (mu_x * w).sum().backward()

    def torch_leg():
        cc = c.clone().requires_grad_(True)
        with torch.device("cuda"):      # (the oracle builds its position tables with the default device)
            _, mu_x, _ = oracle.text_encoder_forward(pr, tok, cc, lens)
        (mu_x * w).sum().backward()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        timed(native); timed(torch_leg)
    tn, tt = [], []
    for _ in range(a.steps):
        tn.append(timed(native)); tt.append(timed(torch_leg))
    print(json.dumps({"workload": "text_encoder_train_step", "B": a.B, "T": a.T, "dt": a.dt, "steps": a.steps,
                      "native_ms_median": round(statistics.median(tn), 3), "torch_fp32_ms_median": round(statistics.median(tt), 3),
                      "ratio_median": round(statistics.median([y / x for x, y in zip(tn, tt)]), 3),
                      "native_ms_min": round(min(tn), 3), "torch_fp32_ms_min": round(min(tt), 3)}))


if __name__ == "__main__":
    main()
