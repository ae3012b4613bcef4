"""Drop-in check against the checkpoint layout of the REAL reference model (CPU).  tests/golden/stabletts_layout.npz holds the
state_dict names and shapes and the decoder's sigma_min of ``StableTTS(401, 128, 256, 1024, 4, 3, 6, 3, 0.1, 256)`` as the
reference's own models/model.py builds it from all-reference modules (oracle/make_golden_dropin.py, which also checks that the
unmodified models/model.py builds around the native modules after ``stabletts_amd.install(text_encoder=True)``).
Here: after install(), the imports of models/model.py:6-7 resolve to the native TextEncoder / CFMDecoder; built with the
arguments models/model.py:36,39 passes, their state_dicts have exactly the names and shapes of the reference model's
``encoder.*`` / ``decoder.*`` entries, and the reference layout loads into them strictly, so released checkpoints load."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stabletts_layout.npz")


def test_native_modules_match_reference_checkpoint_layout():
    import stabletts_amd
    g = np.load(GOLDEN)
    ref = {n: tuple(int(x) for x in s.split(",") if x) for n, s in zip(g["state_dict.names"].tolist(), g["state_dict.shapes"].tolist())}
    n_vocab, mel, hidden, filt, heads, n_enc, n_dec, kernel, p_dropout, gin = (int(v) if v.is_integer() else v for v in g["model_args"].tolist())
    saved = {k: sys.modules.get(k) for k in ("models.flow_matching", "models.text_encoder")}
    try:
        stabletts_amd.install(text_encoder=True)
        TextEncoder = importlib.import_module("models.text_encoder").TextEncoder      # as models/model.py:6-7 import them
        CFMDecoder = importlib.import_module("models.flow_matching").CFMDecoder
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m
    assert TextEncoder.__module__ == "stabletts_amd.text_encoder" and CFMDecoder.__module__ == "stabletts_amd.flow_matching"
    native = {"encoder": TextEncoder(n_vocab, mel, hidden, filt, heads, n_enc, kernel, p_dropout, gin),
              "decoder": CFMDecoder(mel, mel, hidden, mel, filt, heads, n_dec, kernel, p_dropout, gin)}
    gen = torch.Generator().manual_seed(0)
    for prefix, mod in native.items():
        want = {k[len(prefix) + 1:]: s for k, s in ref.items() if k.startswith(prefix + ".")}
        assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == want       # same names, same shapes
        sd = {k: torch.randn(s, generator=gen) for k, s in want.items()}
        missing, unexpected = mod.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
        assert all(torch.equal(mod.state_dict()[k], v) for k, v in sd.items())
    assert native["decoder"].sigma_min == float(g["decoder.sigma_min"])
