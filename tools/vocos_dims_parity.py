#!/usr/bin/env python
"""Parity of the native Vocos vocoder across backbone widths (developer tool; writes profiles/vocos_dims_parity.txt).

    python tools/vocos_dims_parity.py [--parent /path/to/a/library/built/from/the/parent/commit.so]

1. With --parent: dim 512 is unchanged.  The preset (512 / 1536 / 8) on the inputs of tests/golden/vocos_outputs.npz
   (oracle.make_golden_vocos.CASES) through that library and through the in-tree one, both loaded into this process as
   tools/ab_engines.py does: dense and ragged outputs compared bit for bit, f16 and bf16.
2. Accuracy against the float64 oracle, max |audio - ref| / max |ref| over the batch (the metric of tests/test_gpu_vocos.py, bar
   1e-3 for f16), at B = 2, T = 300: the preset, the Vocos trainer's generator (vocoders/vocos/config.py:21-26: 768 / 2048 / 12)
   and 1024 / 2048 / 12, with f16 and bf16 operands, and the trainer's generator through the fp32 training forward."""
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
from stabletts_amd import vocos, vocos_train                               # noqa: E402

OUT = os.path.join(ROOT, "profiles", "vocos_dims_parity.txt")
lines = []


def emit(d):
    lines.append(json.dumps(d))
    print(lines[-1], flush=True)


def make(cfg, sd, dtype, cls=vocos.Vocos):
    m = cls(types.SimpleNamespace(input_channels=cfg.input_channels, dim=cfg.dim, intermediate_dim=cfg.intermediate_dim, num_layers=cfg.num_layers),
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
    sd = vo.make_vocos_state_dict(SD_SEED)
    for dtype in ("f16", "bf16"):
        mods = []
        for path in (parent, default_lib):      # an Engine keeps the CDLL it was created with
            stlib.LIB_PATH, stlib._lib = path, None
            mods.append(make(vo.VocosConfig, sd, dtype))
        stlib.LIB_PATH, stlib._lib = default_lib, None
        for name, (B, T, seed) in CASES.items():
            mel = torch.from_numpy(vo.make_mel(B, T, seed)).cuda()
            lengths = [max(1, T - 3 * b) for b in range(B)]
            dense = [m(mel) for m in mods]
            ragged = [m.forward_ragged(mel, lengths) for m in mods]
            emit({"check": "dim 512: parent build vs this build", "dtype": dtype, "case": name, "B": B, "T": T, "ragged_lengths": lengths,
                  "dense_bitwise_equal": bool(torch.equal(*dense)), "ragged_bitwise_equal": bool(torch.equal(*ragged))})
        B, T = 9, 1001                               # 4 frames per wave in the depthwise kernel, every GEMM on big tiles
        mel = torch.from_numpy(vo.make_mel(B, T, 5)).cuda()
        lengths = [T - 37 * b for b in range(B)]
        emit({"check": "dim 512: parent build vs this build", "dtype": dtype, "case": "R9009", "B": B, "T": T,
              "dense_bitwise_equal": bool(torch.equal(*[m(mel) for m in mods])),
              "ragged_bitwise_equal": bool(torch.equal(*[m.forward_ragged(mel, lengths) for m in mods]))})
        del mods

B, T = 2, 300
for label, over in (("preset 512/1536/8", {}), ("trainer 768/2048/12", dict(dim=768, intermediate_dim=2048, num_layers=12)),
                    ("1024/2048/12", dict(dim=1024, intermediate_dim=2048, num_layers=12))):
    cfg = vo.vocos_config(**over)
    sd = vo.make_vocos_state_dict(SD_SEED, cfg)
    mel_np = vo.make_mel(B, T, 202)
    ref = vo.vocos_forward(sd, mel_np, cfg)
    mel = torch.from_numpy(mel_np).cuda()
    row = {"check": "waveform vs float64 oracle", "generator": label, "B": B, "T": T, "bar_f16": 1e-3}
    for dtype in ("f16", "bf16"):
        row[dtype] = float(f"{rel(make(cfg, sd, dtype)(mel).cpu().numpy(), ref):.3e}")
    tr = make(cfg, sd, "f16", vocos_train.Vocos).train()
    with torch.enable_grad():
        row["fp32_training_forward"] = float(f"{rel(tr(mel).detach().cpu().numpy(), ref):.3e}")
    emit(row)

with open(OUT, "w") as f:
    f.write("# tools/vocos_dims_parity.py on one MI355X (see its docstring)\n" + "\n".join(lines) + "\n")
