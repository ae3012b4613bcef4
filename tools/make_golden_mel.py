"""Generates tests/golden/mel_outputs.npz from the REAL reference feature front end (utils/audio.py, unmodified) and the real
MelStyleEncoder (models/reference_encoder.py).  Run where a checkout of the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_mel.py

torchaudio is absent offline, as torchdiffeq is for the solvers, so utils/audio.py is imported under a stand-in ``torchaudio``
module: its ``transforms.MelScale`` builds the filter bank with stabletts_amd.audio.melscale_fbanks (a restatement of
torchaudio.functional.melscale_fbanks) and projects with torchaudio's own matmul; its ``load`` and ``functional`` raise.  The
filter bank is therefore pinned only against torchaudio's published formula; F.pad, torch.stft, the magnitude, the clamp and the
log run exactly as the reference runs them (CPU, fp32, one thread).

Cases (each stores <case>/cfg = [sample_rate, n_fft, hop_length, pad, n_mels] int64, <case>/wave (B, L) fp32 -- the waveforms
themselves, nothing is regenerated from seeds -- <case>/mel (B, n_mels, frames) and <case>/linear, the LinearSpectrogram output):
  default      MelConfig(), B = 3 speech-like signals (harmonics with vibrato, an envelope, noise); linear of item 0 only
  silence      MelConfig(), digital silence: every magnitude is sqrt(1e-6)
  tone         MelConfig(), a full-scale pure tone without noise: strong bins next to floor-level bins
  edge_pad1    MelConfig(), L = pad + 1;  edge_hop: L a multiple of hop;  edge_odd: L not one
  ms<n_fft>    the seven scales of vocoders/vocos/models/loss.py:11-20 (n_fft 32 ... 2048, hop n_fft / 4, 5 ... 320 mels)
<case>/state_dict lists the reference module's state_dict as "name:shape" strings and <case>/fb_sha256 is the SHA-256 of its fb
bytes (the drop-in must build the same bank), linear_state_dict the same list for LinearSpectrogram; and style_c: the real MelStyleEncoder (weights of tests/synth_weights.py) on the default case's mel, (3, 256) -- the api.py chain
audio -> speaker vector (api.py:73 -> models/model.py:79).
The npz is written with fixed zip timestamps, so regenerating it reproduces the committed file byte for byte.
"""
import hashlib
import io
import os
import sys
import types
import zipfile
from dataclasses import asdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mel_outputs.npz")
MULTI_SCALE = list(zip([5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048]))     # loss.py:11


def _install_torchaudio_standin():
    from stabletts_amd.audio import MelScale as _Restated

    class MelScale(_Restated):
        def forward(self, specgram):            # torchaudio.transforms.MelScale.forward
            return torch.matmul(specgram.transpose(-1, -2), self.fb).transpose(-1, -2)

    def _absent(*a, **k):
        raise RuntimeError("torchaudio stand-in: not available offline")

    ta = types.ModuleType("torchaudio")
    ta.transforms = types.SimpleNamespace(MelScale=MelScale)
    ta.load = _absent
    ta.functional = types.SimpleNamespace(resample=_absent)
    sys.modules["torchaudio"] = ta


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def speech_like(rng, L, sr, f0):
    """Harmonics of a vibrato f0 (5.5 Hz, +-3 %) with 1/h amplitudes, a syllable-rate envelope and white noise."""
    t = np.arange(L) / sr
    phase = 2 * np.pi * np.cumsum(f0 * (1.0 + 0.03 * np.sin(2 * np.pi * 5.5 * t))) / sr
    x = sum(np.sin(h * phase + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 25) if h * f0 < sr / 2)
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t + rng.uniform(0, 2 * np.pi))
    x = x * env + 0.01 * rng.standard_normal(L)
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref_dir, "utils", "audio.py")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, ref_dir)
    torch.set_num_threads(1)
    _install_torchaudio_standin()
    from utils.audio import LogMelSpectrogram, LinearSpectrogram          # reference, unmodified
    from config import MelConfig
    from models.reference_encoder import MelStyleEncoder
    from tests import synth_weights as sw
    assert LogMelSpectrogram.__module__ == "utils.audio"

    rng = np.random.Generator(np.random.PCG64(2024))
    mc = MelConfig()
    sr, pad, hop = mc.sample_rate, mc.pad, mc.hop_length
    cases = {}
    L = int(0.25 * sr)
    cases["default"] = (mc, np.stack([speech_like(rng, L, sr, f0) for f0 in (118.0, 176.0, 231.0)]))
    cases["silence"] = (mc, np.zeros((1, 4096), np.float32))
    cases["tone"] = (mc, np.sin(2 * np.pi * 1234.5 * np.arange(8192) / sr).astype(np.float32)[None])
    for name, n in (("edge_pad1", pad + 1), ("edge_hop", 6 * hop), ("edge_odd", 6 * hop + 137)):
        cases[name] = (mc, speech_like(rng, n, sr, 150.0)[None])
    for n_mels, n_fft in MULTI_SCALE:
        c = MelConfig(n_mels=n_mels, n_fft=n_fft, win_length=n_fft, hop_length=n_fft // 4)
        cases[f"ms{n_fft}"] = (c, speech_like(rng, 3 * n_fft + 11, sr, 140.0)[None])

    out = {}
    with torch.inference_mode():
        for name, (c, wave) in cases.items():
            lm = LogMelSpectrogram(**asdict(c))
            lin = LinearSpectrogram(c.n_fft, c.win_length, c.hop_length, c.pad, c.center, c.pad_mode)
            w = torch.from_numpy(wave)
            out[name + "/cfg"] = np.array([c.sample_rate, c.n_fft, c.hop_length, c.pad, c.n_mels], np.int64)
            out[name + "/wave"] = wave
            out[name + "/mel"] = lm(w).numpy()
            out[name + "/linear"] = lin(w[:1] if name == "default" else w).numpy()
            out[name + "/state_dict"] = np.array([f"{k}:{'x'.join(map(str, v.shape))}" for k, v in lm.state_dict().items()])
            out[name + "/fb_sha256"] = np.array(hashlib.sha256(lm.mel_scale.fb.numpy().tobytes()).hexdigest())
        out["linear_state_dict"] = np.array([f"{k}:{'x'.join(map(str, v.shape))}" for k, v in lin.state_dict().items()])
        style = MelStyleEncoder(sw.N_MELS, style_vector_dim=sw.GIN, style_kernel_size=5, dropout=0.25).eval()
        style.load_state_dict(sw.style_encoder_state_dict(), strict=True)
        out["style_c"] = style(torch.from_numpy(out["default/mel"]), None).numpy()
    _save(OUT, out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} kB): " + ", ".join(f"{k}{list(v.shape)}" for k, v in out.items() if k.endswith("/mel")))
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
