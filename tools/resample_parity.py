"""Records the parity figures of the native sinc resampler (stabletts_amd.audio.resample) on an MI355X: per configuration and
input shape of tests/test_gpu_resample.py, the max-abs error of the native kernel and of the module's own fp32 dense fallback
(F.pad + conv1d, same GPU) against the float64 dense restatement (tests/resample_restatement.py), the floor 2^-24 max|y|, and
ratio = native / max(torch fp32, floor) (bar 4).

    python tools/resample_parity.py [--out profiles/resample_parity.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_parity.txt"))
    a = ap.parse_args()
    import torch

    from stabletts_amd.audio import resample_table
    from tests import resample_restatement as R
    from tests import test_gpu_resample as T
    chunk = T._chunk()
    lines = [f"# python tools/resample_parity.py   (one MI355X; chunk = {chunk} output samples per block)",
             "# error = max-abs against the float64 dense restatement; floor = 2^-24 max|y|; ratio = native / max(torch fp32, floor) (bar 4)"]
    worst = 0.0
    with torch.no_grad():
        for (o, n, kw), name in zip(R.CONFIGS, R.IDS):
            S = resample_table(o, n, **kw)["S"]
            for shape, e_native, e_torch, floor in T.parity_errors(o, n, kw, chunk):
                ratio = e_native / max(e_torch, floor)
                worst = max(worst, ratio)
                lines.append(f"{name:20s} S {S:3d}  x {str(shape):14s} native {e_native:.3e}  torch fp32 {e_torch:.3e}  floor {floor:.3e}  ratio {ratio:5.2f}")
    lines.append(f"# worst ratio {worst:.2f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
