#!/usr/bin/env python
"""Parity of the native Vocos vocoder across ISTFT sizes and mel widths (developer tool; writes profiles/vocos_rates_parity.txt).

    python tools/vocos_rates_parity.py [--parent /path/to/a/library/built/from/the/parent/commit.so]

1. With --parent: what the parent commit accepted is unchanged.  The preset (n_fft 2048 / hop 512, M = 128) and the same generator at
   M = 64 and M = 192, on the inputs of tests/golden/vocos_outputs.npz (oracle.make_golden_vocos.CASES, the mel at the handle's width)
   and on one batch of 9 x 1001 frames, through that library and through the in-tree one, both loaded into this process as
   tools/ab_engines.py does: dense and ragged outputs compared bit for bit, f16 and bf16.
2. Accuracy against the float64 oracle, max |audio - ref| / max |ref| over the batch (the metric of tests/test_gpu_vocos.py, bar 1e-3
   for f16, 1e-2 for bf16), at B = 2, T = 300 with the preset's backbone (512 / 1536 / 8): n_fft 2048 / 1024 / 512 / 256 at M = 128 and
   at the mel widths of 16-24 kHz models (80, 96, 16, 176), with f16 and bf16 operands.  The n_fft 2048, M = 128 row is the preset: a
   new configuration that misses the bar while that row passes it is a finding.
3. The ISTFT alone at each n_fft: audio against the float64 istft_same of the captured head output (bar 2e-5)."""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vocos_oracle as vo                                      # noqa: E402
from oracle.make_golden_vocos import CASES, SD_SEED                        # noqa: E402
from stabletts_amd import _lib as stlib                                    # noqa: E402
from stabletts_amd import vocos                                            # noqa: E402

OUT = os.path.join(ROOT, "profiles", "vocos_rates_parity.txt")
lines = []


def emit(d):
    lines.append(json.dumps(d))
    print(lines[-1], flush=True)


def make(cfg, sd, dtype):
    m = vocos.Vocos(types.SimpleNamespace(input_channels=cfg.input_channels, dim=cfg.dim, intermediate_dim=cfg.intermediate_dim, num_layers=cfg.num_layers),
                    types.SimpleNamespace(n_fft=cfg.n_fft, hop_length=cfg.hop_length), operand_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.cuda()
    m.engine()
    return m


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
if parent:
    default_lib = stlib.LIB_PATH
    for M in (128, 64, 192):
        cfg = vo.vocos_config(input_channels=M)
        sd = vo.make_vocos_state_dict(SD_SEED, cfg)
        for dtype in ("f16", "bf16"):
            mods = []
            for path in (parent, default_lib):      # an Engine keeps the CDLL it was created with
                stlib.LIB_PATH, stlib._lib = path, None
                mods.append(make(cfg, sd, dtype))
            stlib.LIB_PATH, stlib._lib = default_lib, None
            dense_eq, ragged_eq = [], []
            for name, (B, T, seed) in {**CASES, "R9009": (9, 1001, 5)}.items():
                mel = torch.from_numpy(vo.make_mel(B, T, seed, M)).cuda()
                lengths = [max(1, T - 3 * b) for b in range(B)]
                dense_eq.append(bool(torch.equal(*[m(mel) for m in mods])))
                ragged_eq.append(bool(torch.equal(*[m.forward_ragged(mel, lengths) for m in mods])))
            emit({"check": "n_fft 2048 / hop 512: parent build vs this build", "input_channels": M, "dtype": dtype,
                  "cases": list(CASES) + ["R9009"], "dense_bitwise_equal": dense_eq, "ragged_bitwise_equal": ragged_eq,
                  "all_bitwise_equal": all(dense_eq) and all(ragged_eq)})
            del mods

B, T = 2, 300
for n_fft, M in ((2048, 128), (1024, 128), (512, 128), (256, 128), (2048, 80), (1024, 80), (512, 96), (256, 16), (256, 176)):
    cfg = vo.vocos_config(n_fft=n_fft, hop_length=n_fft // 4, input_channels=M)
    sd = vo.make_vocos_state_dict(SD_SEED, cfg)
    mel_np = vo.make_mel(B, T, 202, M)
    ref = vo.vocos_forward(sd, mel_np, cfg)
    mel = torch.from_numpy(mel_np).cuda()
    row = {"check": "waveform vs float64 oracle", "n_fft": n_fft, "hop_length": n_fft // 4, "input_channels": M, "generator": "512/1536/8",
           "B": B, "T": T, "bar_f16": 1e-3, "bar_bf16": 1e-2}
    for dtype in ("f16", "bf16"):
        row[dtype] = float(f"{rel(make(cfg, sd, dtype)(mel).cpu().numpy(), ref):.3e}")
    emit(row)

B, T = 3, 61
for n_fft in (2048, 1024, 512, 256):
    cfg = vo.vocos_config(n_fft=n_fft, hop_length=n_fft // 4)
    sd = vo.make_vocos_state_dict(SD_SEED, cfg)
    m = make(cfg, sd, "f16")
    eng = m.engine()
    eng.debug_capture(True)
    audio = m(torch.from_numpy(vo.make_mel(B, T, 11)).cuda()).cpu().numpy()
    ho = eng.debug_fetch("voc.head_out").reshape(B, T, 2, -1)[..., :n_fft // 2 + 1].astype(np.float64)
    eng.debug_capture(False)
    S = (np.minimum(np.exp(ho[:, :, 0]), 1e2) * (np.cos(ho[:, :, 1]) + 1j * np.sin(ho[:, :, 1]))).transpose(0, 2, 1)
    ref = vo.istft_same(S, sd["head.istft.window"].astype(np.float64), n_fft, n_fft // 4)
    emit({"check": "ISTFT alone vs float64 istft of the captured head output", "n_fft": n_fft, "B": B, "T": T, "bar": 2e-5,
          "max_rel": float(f"{rel(audio, ref):.3e}")})

with open(OUT, "w") as f:
    f.write("# tools/vocos_rates_parity.py on one MI355X (see its docstring)\n" + "\n".join(lines) + "\n")
