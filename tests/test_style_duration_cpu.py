"""MelStyleEncoder / DurationPredictor drop-ins on a CPU-only box: after install(reference_encoder=True,
duration_predictor=True) the imports of models/model.py:8-9 resolve to the native classes; built with the arguments of
models/model.py:38-39 they have exactly the ``ref_encoder.*`` / ``dp.*`` names and shapes of the REAL reference model
(tests/golden/stabletts_layout.npz) and load that layout strictly; the new C entry points exist, reject NULL arguments and
handles of the other kinds; duration_loss is the reference's arithmetic."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stabletts_layout.npz")


@pytest.fixture(scope="module")
def lib():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    return _lib.load()


def _installed():
    import stabletts_amd
    names = ("models.flow_matching", "models.reference_encoder", "models.duration_predictor")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        stabletts_amd.install(reference_encoder=True, duration_predictor=True)
        return (importlib.import_module("models.reference_encoder").MelStyleEncoder,
                importlib.import_module("models.duration_predictor"))
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m


def test_modules_match_reference_checkpoint_layout():
    MelStyleEncoder, dpmod = _installed()
    assert MelStyleEncoder.__module__ == "stabletts_amd.reference_encoder"
    assert dpmod.DurationPredictor.__module__ == "stabletts_amd.duration_predictor" and callable(dpmod.duration_loss)
    g = np.load(GOLDEN)
    ref = {n: tuple(int(x) for x in s.split(",") if x) for n, s in zip(g["state_dict.names"].tolist(), g["state_dict.shapes"].tolist())}
    n_vocab, mel, hidden, filt, heads, n_enc, n_dec, kernel, p_dropout, gin = (int(v) if v.is_integer() else v for v in g["model_args"].tolist())
    native = {"ref_encoder": MelStyleEncoder(mel, style_vector_dim=gin, style_kernel_size=5, dropout=0.25),    # model.py:38
              "dp": dpmod.DurationPredictor(hidden, filt, kernel, 0.5, gin)}                                  # model.py:39
    counts = {"ref_encoder": 460288, "dp": 4005121}
    gen = torch.Generator().manual_seed(0)
    for prefix, mod in native.items():
        want = {k[len(prefix) + 1:]: s for k, s in ref.items() if k.startswith(prefix + ".")}
        assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == want
        assert sum(p.numel() for p in mod.parameters()) == counts[prefix]
        sd = {k: torch.randn(s, generator=gen) for k, s in want.items()}
        missing, unexpected = mod.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
        assert all(torch.equal(mod.state_dict()[k], v) for k, v in sd.items())


def test_install_leaves_other_modules_alone():
    import stabletts_amd
    saved = {k: sys.modules.get(k) for k in ("models.flow_matching", "models.reference_encoder", "models.duration_predictor")}
    try:
        sys.modules.pop("models.reference_encoder", None)
        sys.modules.pop("models.duration_predictor", None)
        stabletts_amd.install()
        assert "models.reference_encoder" not in sys.modules and "models.duration_predictor" not in sys.modules
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m
    assert stabletts_amd.MelStyleEncoder.__name__ == "MelStyleEncoder"
    assert stabletts_amd.DurationPredictor.__name__ == "DurationPredictor"


def test_duration_loss_matches_reference_arithmetic():
    from stabletts_amd.duration_predictor import duration_loss
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(2, 1, 9, generator=g), torch.randn(2, 1, 9, generator=g)
    lengths = torch.tensor([9, 4])
    assert torch.allclose(duration_loss(a, b, lengths), torch.sum((a - b) ** 2) / torch.sum(lengths))


def test_new_symbols_reject_null_and_wrong_kind(lib):
    from stabletts_amd._lib import StDurationPredictorConfig, StStyleEncoderConfig
    h = ctypes.c_void_p()
    assert lib.st_create_style_encoder(None, 0, ctypes.byref(h)) == -1
    assert lib.st_create_duration_predictor(None, 0, ctypes.byref(h)) == -1
    assert lib.st_create_style_encoder(ctypes.byref(StStyleEncoderConfig(128, 128, 256, 5, 2)), 0, None) == -1
    assert lib.st_create_duration_predictor(ctypes.byref(StDurationPredictorConfig(256, 1024, 3, 256)), 0, None) == -1
    assert lib.st_style_encoder_forward(None, None, None, None, 1, 1, None) == -1
    assert lib.st_duration_predictor_forward(None, None, None, None, None, 1, 1, None) == -1


def test_create_validates_configs(lib):
    from stabletts_amd._lib import StDurationPredictorConfig, StStyleEncoderConfig
    h = ctypes.c_void_p()

    def se(*a):
        return lib.st_create_style_encoder(ctypes.byref(StStyleEncoderConfig(*a)), 0, ctypes.byref(h)), lib.st_last_error(None).decode()

    def dp(*a):
        return lib.st_create_duration_predictor(ctypes.byref(StDurationPredictorConfig(*a)), 0, ctypes.byref(h)), lib.st_last_error(None).decode()

    assert se(128, 128, 256, 5, 3)[0] == -1                  # embed_dim % num_heads != 0: the reference raises too
    assert se(128, 128, 256, 5, 4)[0] == -4                  # head_dim 32: valid in the reference, not built natively
    assert se(128, 128, 256, 4, 2)[0] == -4
    assert dp(256, 1000, 3, 256)[0] == -4                    # filter_channels not a multiple of 128
    assert dp(256, 1024, 2, 256)[0] == -4
    assert dp(0, 1024, 3, 256)[0] == -1
    if not torch.cuda.is_available():                        # a supported config reaches the device check
        rc, msg = se(128, 128, 256, 5, 2)
        assert rc == -2 and "device" in msg
        rc, msg = dp(256, 1024, 3, 256)
        assert rc == -2 and "device" in msg


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-box behaviour")
def test_no_gpu_fails_loudly():
    from stabletts_amd.duration_predictor import DurationPredictor
    from stabletts_amd.reference_encoder import MelStyleEncoder
    se = MelStyleEncoder(128, style_vector_dim=256, style_kernel_size=5, dropout=0.25)
    dp = DurationPredictor(256, 1024, 3, 0.5, 256)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            se(torch.zeros(1, 128, 8))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dp(torch.zeros(1, 256, 8), torch.ones(1, 1, 8), torch.zeros(1, 256))
