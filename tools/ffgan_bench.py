"""Times the native FireflyGAN vocoder (stabletts_amd.ffgan.FireflyGANBase, default configuration, seeded weights) against the
restatement of tests/ffgan_restatement.py run as a torch module on the same GPU: in fp32, and under fp16 autocast.

    python tools/ffgan_bench.py [--out profiles/ffgan_bench.txt]
    python tools/ffgan_bench.py --ragged [--out profiles/ffgan_ragged_bench.txt]

Shapes: B = 1 x T = 1000 and B = 32 x T = 1000 mel frames (512 samples each).  Per shape and implementation: the median of the timed
calls (HIP events around each call, after warm-up), the achieved TFLOP/s on the model's FLOPs (2 x multiply-adds of every conv and
linear; the zero taps of the polyphase transposed convs are not counted) and, for the native path, the TB/s on the bytes its
launches must move at least (every launch reads its inputs and writes its outputs once; weights not counted).

--ragged: one bucket of 32 utterances of U{600..1000} frames (seed 4), f16, as the padded dense call, the ragged call
(FireflyGANBase.forward_ragged) and a loop of 32 single-utterance calls, and the ragged call with every length equal to T beside two
runs of the dense call (their difference is the run-to-run spread).  Legs in turn within a round, median over the rounds.

--operand-dtype (default f16; f16_split / bf16_split: the hi + lo operand pairs): without --ragged the named handle is timed beside
the f16 and bf16 ones in the same run; with --ragged it is the bucket's handle and, if it is not f16, the dense and ragged legs of an
f16 handle of the same build run in the same rounds.  Without the flag the output is what it was before the flag existed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model_flops_per_frame(cfg):
    b, h = cfg["backbone"], cfg["head"]
    K = b["kernel_size"]
    f = 2.0 * b["dims"][0] * b["input_channels"] * K
    for i, C in enumerate(b["dims"]):
        if i:
            f += 2.0 * C * b["dims"][i - 1]
        f += b["depths"][i] * (2.0 * C * K + 2 * 2.0 * C * 4 * C)
    C0 = h["upsample_initial_channel"]
    f += 2.0 * C0 * h["num_mels"] * h["pre_conv_kernel_size"]
    up = 1
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        ci, co = C0 >> i, C0 >> (i + 1)
        up *= u
        f += up * 2.0 * ci * co * (k // u)                      # every output sample sees k / u taps
        for rk, dil in zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]):
            f += up * len(dil) * 2 * 2.0 * co * co * rk
    f += up * 2.0 * (C0 >> len(h["upsample_rates"])) * h["post_conv_kernel_size"]
    return f


def native_bytes_per_frame(cfg):
    """Lower bound of the HBM traffic of the native launch sequence (engine_ffgan.cpp), bytes per mel frame."""
    b, h = cfg["backbone"], cfg["head"]
    M = b["input_channels"]
    n = M * 4 + 7 * M * 2 * 2 + b["dims"][0] * 4 * 3                       # im2col, stem GEMM, LayerNorm in place
    for i, C in enumerate(b["dims"]):
        if i:
            n += b["dims"][i - 1] * (4 + 2 + 2) + C * 4                     # LayerNorm -> 16 bit, k = 1 conv
        n += b["depths"][i] * (C * (4 + 2) + C * 2 + 4 * C * 2 + 4 * C * 2 + C * 8)      # dwconv + LN, pwconv1, pwconv2 + residual
    D, C0 = b["dims"][-1], h["upsample_initial_channel"]
    n += D * (4 + 4 + 2) + D * 2 + C0 * 4
    up = 1
    for i, u in enumerate(h["upsample_rates"]):
        ci, co = C0 >> i, C0 >> (i + 1)
        n += up * ci * 4 + up * u * co * 4                                  # transposed conv: fp32 in, fp32 out
        up *= u
        pairs = sum(len(d) for d in h["resblock_dilation_sizes"])
        n += up * co * pairs * ((4 + 2) + (2 + 4 + 4))                      # c1: fp32 in, 16 bit out; c2: 16 bit in, residual in, fp32 out
        n += up * co * 4 * (len(h["resblock_kernel_sizes"]) - 1)            # the mean's read-modify-write of blocks 1..
    n += up * (C0 >> len(h["upsample_rates"])) * 4 + up * 4
    return float(n)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def ragged_bucket(out, dt="f16"):
    """Host clock around CALLS calls that end in a device synchronise; in a round every leg runs in turn, so that drift of a shared
    machine lands on all of them."""
    import numpy as np
    from tests import ffgan_restatement as R
    from stabletts_amd.ffgan import FireflyGANBase
    ROUNDS, CALLS, NB = 9, 2, 32
    m = FireflyGANBase(operand_dtype=dt)
    m.load_state_dict(R.make_state_dict(R.DEFAULT, R.SEED), strict=True)
    m = m.cuda().eval()
    lengths = np.random.default_rng(4).integers(600, 1001, NB).tolist()
    Tmax, rows = max(lengths), sum(lengths)
    mel = R.make_mel(NB, Tmax, 128, 3).cuda()
    for b, n in enumerate(lengths):
        mel[b, :, n:] = 0.0
    solo = [mel[b:b + 1, :, :n].contiguous() for b, n in enumerate(lengths)]
    full = [Tmax] * NB
    legs = {"dense_padded": lambda: m(mel), "ragged": lambda: m.forward_ragged(mel, lengths),
            "solo_loop": lambda: [m(x) for x in solo],
            "dense_a": lambda: m(mel), "ragged_equal_lengths": lambda: m.forward_ragged(mel, full), "dense_b": lambda: m(mel)}
    if dt != "f16":                   # the default handle of the same build in the same rounds
        f16 = FireflyGANBase(operand_dtype="f16")
        f16.load_state_dict(R.make_state_dict(R.DEFAULT, R.SEED), strict=True)
        f16 = f16.cuda().eval()
        legs.update({"f16_dense_padded": lambda: f16(mel), "f16_ragged": lambda: f16.forward_ragged(mel, lengths)})
    for fn in legs.values():          # every shape of the timed window, twice
        fn(); fn()
    ms = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize(); ms[k].append((time.perf_counter() - t0) / CALLS * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = abs(med["dense_a"] - med["dense_b"]) / med["dense_a"]
    lines = [
        {"workload": "ffgan_bucket", "dtype": dt, "B": NB, "Tmax": Tmax, "packed_rows": rows, "padded_rows": NB * Tmax,
         "rows_ratio": round(rows / (NB * Tmax), 3), "rounds": ROUNDS, "calls_per_round": CALLS,
         "dense_padded_ms_median": round(med["dense_padded"], 3), "ragged_ms_median": round(med["ragged"], 3),
         "solo_loop_ms_median": round(med["solo_loop"], 3), "ragged_over_dense": round(med["ragged"] / med["dense_padded"], 3),
         "ragged_over_solo_loop": round(med["ragged"] / med["solo_loop"], 3)},
        {"workload": "ffgan_equal_lengths", "dtype": dt, "B": NB, "T": Tmax, "rows": NB * Tmax,
         "dense_a_ms_median": round(med["dense_a"], 3), "dense_b_ms_median": round(med["dense_b"], 3),
         "ragged_equal_lengths_ms_median": round(med["ragged_equal_lengths"], 3),
         "dense_run_to_run": round(spread, 4), "ragged_over_dense_a": round(med["ragged_equal_lengths"] / med["dense_a"], 4)},
    ]
    if dt != "f16":
        lines.append({"workload": "ffgan_bucket_vs_f16", "dtype": dt, "f16_dense_padded_ms_median": round(med["f16_dense_padded"], 3),
                      "f16_ragged_ms_median": round(med["f16_ragged"], 3), "dense_over_f16": round(med["dense_padded"] / med["f16_dense_padded"], 3),
                      "ragged_over_f16": round(med["ragged"] / med["f16_ragged"], 3)})
    head = ("# tools/ffgan_bench.py --ragged on one MI355X: one bucket of 32 utterances of U{600..1000} frames (seed 4) through the native\n"
            "# FireflyGAN vocoder (default configuration) as the padded dense call (FireflyGANBase.forward: wrong for every utterance shorter\n"
            "# than the longest), the ragged call (forward_ragged) and a loop of 32 single-utterance dense calls; and the ragged call with every\n"
            "# length equal to T beside two runs of the dense call at the same rows (their difference is the run-to-run spread).  ms per call,\n"
            "# host clock around calls_per_round calls ending in a device synchronise, legs in turn within a round, median over the rounds.\n")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(head)
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1x1000,32x1000")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--operand-dtype", default="f16", choices=["f16", "bf16", "f16_split", "bf16_split"])
    args = ap.parse_args()
    tag = "" if args.operand_dtype == "f16" else "_" + args.operand_dtype
    if args.ragged:
        return ragged_bucket(args.out or os.path.join(ROOT, "profiles", f"ffgan_ragged_bench{tag}.txt"), args.operand_dtype)
    args.out = args.out or os.path.join(ROOT, "profiles", f"ffgan_bench{tag}.txt")
    from tests import ffgan_restatement as R
    from stabletts_amd.ffgan import FireflyGANBase
    cfg = R.DEFAULT
    sd = R.make_state_dict(cfg, R.SEED)
    native = {}
    dts = ("f16", "bf16") + ((args.operand_dtype,) if args.operand_dtype not in ("f16", "bf16") else ())
    for dt in dts:
        m = FireflyGANBase(operand_dtype=dt)
        m.load_state_dict(sd, strict=True)
        native[dt] = m.cuda().eval()
    W32 = R.prepare(sd, dtype=torch.float32, device="cuda")
    fl, by = model_flops_per_frame(cfg), native_bytes_per_frame(cfg)
    lines = [f"FireflyGANBase, default configuration: {fl / 1e9:.3f} GFLOP and >= {by / 1e6:.2f} MB of native HBM traffic per mel frame",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median (min .. max) ms per call", ""]
    for shape in args.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        mel = R.make_mel(B, T, 128, 9).cuda()
        big = B * T >= 8000
        warm, iters = (2, 5) if big else (5, 20)

        def torch32():
            with torch.no_grad():
                return R.forward(None, cfg, mel, prepared=W32)["audio"]

        def torch16():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return R.forward(None, cfg, mel, prepared=W32)["audio"]

        rows = [(f"native {dt}", (lambda m=native[dt]: m(mel))) for dt in dts] + [("torch fp32", torch32), ("torch fp16 autocast", torch16)]
        ref = torch32().double()
        lines.append(f"B = {B} x T = {T}: {fl * B * T / 1e12:.2f} TFLOP")
        for name, fn in rows:
            med, lo, hi = timed(fn, warm, iters)
            err = float((fn().double() - ref).abs().max() / ref.abs().max())
            extra = f"  {by * B * T / med / 1e9:6.2f} TB/s" if name.startswith("native") and "split" not in name else ""      # (by: the 16-bit sequence's bytes)
            lines.append(f"  {name:<20} {med:9.2f} ms ({lo:.2f} .. {hi:.2f})  {fl * B * T / med / 1e9:7.1f} TFLOP/s{extra}   max |audio - torch fp32| / max = {err:.1e}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
