"""Generates tests/golden/mel_loss_grads.npz from the REAL reference Vocos multi-scale mel loss (vocoders/vocos/models/loss.py,
unmodified: seven utils/audio.py LogMelSpectrogram modules, n_fft 32 ... 2048, L1 summed), the unit vocoders/vocos/train.py:115
differentiates.  Run where a checkout of the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_mel_loss.py

utils/audio.py runs under the torchaudio stand-in of tools/make_golden_mel.py (imported from there), on the CPU, one thread.
Inputs: two speech-like batches x (the generator's output, which requires grad) and y (the target), B = 2 x 8192 samples each in
the (B, 1, L) form train.py passes.  Stored: x, y (B, 1, L) fp32; loss32 and dx32 = dL/dx of the fp32 module; loss64 and dx64 of
the same module in float64 (.double()).  The npz is written with fixed zip timestamps, so regenerating it reproduces the committed
file byte for byte.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mel_loss_grads.npz")


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE", "/root/reference")
    loss_py = os.path.join(ref_dir, "vocoders", "vocos", "models", "loss.py")
    if not os.path.isfile(loss_py):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ref_dir)
    torch.set_num_threads(1)
    from make_golden_mel import _install_torchaudio_standin, _save, speech_like
    _install_torchaudio_standin()
    spec = importlib.util.spec_from_file_location("vocos_loss", loss_py)
    loss_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(loss_mod)                                 # reference, unmodified
    assert loss_mod.LogMelSpectrogram.__module__ == "utils.audio"

    rng = np.random.Generator(np.random.PCG64(115))
    sr, L = 44100, 8192
    x = np.stack([speech_like(rng, L, sr, f0) for f0 in (132.0, 207.0)])[:, None]
    y = np.stack([speech_like(rng, L, sr, f0) for f0 in (128.0, 214.0)])[:, None]
    out = {"x": x, "y": y}
    loss_fn = loss_mod.MultiScaleMelSpectrogramLoss()
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        fn = loss_fn.to(dt)
        xt = torch.from_numpy(x).to(dt).requires_grad_(True)
        loss = fn(xt, torch.from_numpy(y).to(dt))
        loss.backward()
        out["loss" + tag] = np.array(loss.item(), np.float32 if tag == "32" else np.float64)
        out["dx" + tag] = xt.grad.numpy()
    _save(OUT, out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} kB): loss fp32 {float(out['loss32']):.6f}, float64 {float(out['loss64']):.9f}; "
          f"dx fp32 vs float64 rel L2 {np.linalg.norm(out['dx32'] - out['dx64']) / np.linalg.norm(out['dx64']):.2e}")
    assert os.path.getsize(OUT) < 400 * 1000


if __name__ == "__main__":
    main()
