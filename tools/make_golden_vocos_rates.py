"""Generates tests/golden/vocos_rates.npz: the REAL reference Vocos generator (vocoders/vocos/models/model.py, unmodified, CPU, one
thread, float64) at the ISTFT sizes and mel widths of 16-24 kHz models, in the manner of tools/make_golden_vocos_dims.py.  Run
where a checkout of the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_vocos_rates.py

Cases: tests/vocos_rates_cases.CASES -- (n_fft, hop, M, dim) = (1024, 256, 80, 512), (512, 128, 96, 768), (256, 64, 16, 1024), each with
intermediate_dim 256 and 1-2 layers.  The module is Vocos(VocosConfig(M, dim, F, layers), MelConfig(n_fft=N, win_length=N,
hop_length=N // 4, n_mels=M)), its weights make_vocos_state_dict(seed, cfg), its input make_mel.  Stored per case: audio64, the
float64 waveform (B, T * hop) whole.  The generator asserts that no log-magnitude lies within 1e-4 of the head's clip at ln 100.
Fixed zip timestamps: regenerating the file reproduces it byte for byte.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "vocos_rates.npz")


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE", "")
    if not os.path.isfile(os.path.join(ref_dir, "vocoders", "vocos", "models", "model.py")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ref_dir)
    torch.set_num_threads(1)
    from make_golden_mel import _install_torchaudio_standin, _save
    _install_torchaudio_standin()
    from config import MelConfig, VocosConfig
    from vocoders.vocos.models.model import Vocos                     # reference, unmodified
    from oracle import vocos_oracle as vo
    from tests import vocos_rates_cases as D

    res = {}
    for case, (fields, B, T, wseed, mseed) in D.CASES.items():
        cfg = vo.vocos_config(**fields)
        sd = vo.make_vocos_state_dict(wseed, cfg)
        voc = Vocos(VocosConfig(cfg.input_channels, cfg.dim, cfg.intermediate_dim, cfg.num_layers),
                    MelConfig(n_fft=cfg.n_fft, win_length=cfg.n_fft, hop_length=cfg.n_fft // 4, n_mels=cfg.input_channels))
        voc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        voc = voc.to(torch.float64)
        near = []
        hook = voc.head.out.register_forward_hook(
            lambda m, i, o: near.append(float((o[..., :o.shape[-1] // 2].detach() - np.log(100.0)).abs().min())))
        with torch.no_grad():
            audio = voc(torch.from_numpy(vo.make_mel(B, T, mseed, M=cfg.input_channels)).to(torch.float64))
        hook.remove()
        assert near[0] > 1e-4, f"{case}: a log-magnitude lies {near[0]:.1e} from the clip"
        assert tuple(audio.shape) == (B, T * cfg.hop_length), (case, tuple(audio.shape))
        res[f"{case}/audio64"] = audio.numpy()
        print(case, tuple(audio.shape), "max |audio|", float(audio.abs().max()), "nearest to the clip", near[0])
    _save(OUT, res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 400 * 1000


if __name__ == "__main__":
    main()
