"""Times the native sinc resampler (stabletts_amd.audio.resample / resample_ragged, st_resample) against the module's own dense
fallback (torchaudio's formulation: F.pad + a strided conv1d over the dense kernel) in fp32 on the same GPU:

  batch    B = 32 waveforms of 10 s, one call each side, at 48000 -> 44100, 24000 -> 44100, 16000 -> 44100 and 44100 -> 16000
  ragged   256 files of 2 .. 12 s (seeded lengths, in steps of half a second so that the convolution library behind the dense
           side meets 21 shapes, not 256) at the same conversions: one resample_ragged call natively, one dense call per file on
           the other side (the dense form has no ragged batch)

After a warm-up of every shape the two sides alternate; each sample times `--calls` back-to-back calls between two device
events (host and device: what a caller waits for).  Prints one JSON line per case: the medians in ms per call with the 10th and
90th percentiles, the median of the paired ratios, the device-busy time of one call of each side (torch.profiler: kernels, fills
and copies) and what 4 (L_in + L_out) bytes -- every sample read once and written once -- over those times comes to, against the
MI355X's HBM rate (8.0 TB/s peak, 6.29 TB/s measured for a float4 copy).  The B = 32 batch moves 0.1 GB, which fits the 256 MB
Infinity Cache: a GB/s above the HBM rate there is the cache's.

    python tools/resample_bench.py [--reps 20] [--warmup 3] [--calls 5] [--out profiles/resample_bench.txt]
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONVERSIONS = [(48000, 44100), (24000, 44100), (16000, 44100), (44100, 16000)]
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def _timed(f, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def _busy_ms(f):
    from torch.profiler import ProfilerActivity, profile
    f()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        f()
        torch.cuda.synchronize()
    rows = prof.key_averages()
    return sum(r.count for r in rows), sum(getattr(r, "self_device_time_total", None) or getattr(r, "self_cuda_time_total", 0) for r in rows) / 1e3


def _pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def _case(name, o, n, native, dense, n_bytes, a, check):
    for _ in range(a.warmup):
        native()
        dense()
    torch.cuda.synchronize()
    e = check()
    times = {"native": [], "dense": []}
    for _ in range(a.reps):
        times["native"].append(_timed(native, a.calls))
        times["dense"].append(_timed(dense, a.calls))
    out = {"case": name, "orig_freq": o, "new_freq": n, "mbytes_at_4B_in_plus_out": round(n_bytes / 1e6, 1), "reps": a.reps, "calls_per_rep": a.calls,
           "native_vs_dense_max_abs": e}
    for k, v in times.items():
        out[k + "_ms_median"] = round(statistics.median(v), 4)
        out[k + "_ms_p10_p90"] = [round(_pct(v, 0.1), 4), round(_pct(v, 0.9), 4)]
    out["dense_over_native_median_of_pairs"] = round(statistics.median([d / x for x, d in zip(times["native"], times["dense"])]), 2)
    for k, f in (("native", native), ("dense", dense)):
        out[k + "_launches"], busy = _busy_ms(f)
        out[k + "_device_busy_ms"] = round(busy, 4)
    for k in ("native_ms_median", "native_device_busy_ms"):
        rate = n_bytes / (out[k] * 1e-3)
        out[k.replace("_ms_median", "_call").replace("_device_busy_ms", "_device_busy") + "_gbytes_per_s"] = round(rate / 1e9, 1)
    out["native_device_busy_share_of_hbm_peak_and_copy"] = [round(n_bytes / (out["native_device_busy_ms"] * 1e-3) / r, 3) for r in (HBM_PEAK, HBM_COPY)]
    return json.dumps(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.txt"))
    a = ap.parse_args()
    from stabletts_amd import audio
    assert torch.cuda.is_available(), "resample_bench needs a HIP device"
    dev = "cuda:0"
    lines = [f"# python tools/resample_bench.py --reps {a.reps} --warmup {a.warmup} --calls {a.calls}   (one MI355X, fp32; ms per call, host and device)"]
    gen = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for o, n in CONVERSIONS:
            key = audio._resample_key(o, n, 6, 0.99, "sinc_interp_hann", None)
            x = torch.randn(32, 10 * o, device=dev, generator=gen)
            n_bytes = 4 * (x.numel() + 32 * audio._out_len(10 * o, key[0], key[1]))
            lines.append(_case("batch 32 x 10 s", o, n, lambda: audio.resample(x, o, n), lambda: audio._resample_dense(x, key), n_bytes, a,
                               lambda: float((audio.resample(x, o, n) - audio._resample_dense(x, key)).abs().max())))
            print(lines[-1], flush=True)
            del x
            rnd = random.Random(1)
            files = [torch.randn(rnd.randint(4, 24) * o // 2, device=dev, generator=gen) for _ in range(256)]
            n_bytes = 4 * sum(f.numel() + audio._out_len(f.numel(), key[0], key[1]) for f in files)
            lines.append(_case("ragged 256 files of 2 .. 12 s", o, n, lambda: audio.resample_ragged(files, o, n),
                               lambda: [audio._resample_dense(f, key) for f in files], n_bytes, a,
                               lambda: max(float((p - q).abs().max()) for p, q in zip(audio.resample_ragged(files, o, n),
                                                                                      [audio._resample_dense(f, key) for f in files]))))
            print(lines[-1], flush=True)
            del files
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
