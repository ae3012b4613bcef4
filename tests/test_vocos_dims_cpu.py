"""CPU checks of the Vocos widths 768 and 1024 (the Vocos trainer's own generator is 128 / 768 / 2048 / 12,
vocoders/vocos/config.py:21-26): the creation limits of st_create_vocoder, the float64 oracle's forward and the restatement's VJP
pinned to the REAL reference module at those widths (tests/golden/vocos_dims.npz, tools/make_golden_vocos_dims.py), and the
module's state_dict at the trainer's configuration."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from oracle import vocos_oracle as vo
from tests import vocos_dims_cases as D
from tests import vocos_vjp_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vocos_dims.npz")
BAR = 1e-10         # tests/test_vocos_backward_cpu.py: both sides are float64 evaluations of the same formulas


@pytest.fixture(scope="module")
def lib():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _rel_l2(a, ref):
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def test_creation_accepts_dim_512_768_1024_and_no_other(lib):
    """dim 768 and 1024 pass the limits (on a box without a GPU creation then ends in ST_ERR_HIP, with one in ST_OK); every other
    width is ST_ERR_UNSUPPORTED with a message that names the three, before any device is touched; dim 0 stays ST_ERR_INVALID."""
    from stabletts_amd._lib import StVocosConfig, ST_ERR_HIP, ST_ERR_INVALID, ST_ERR_UNSUPPORTED, ST_OK
    ok = dict(input_channels=128, dim=512, intermediate_dim=1536, num_layers=8, n_fft=2048, hop_length=512, operand_dtype=0)
    for dim in (768, 1024):
        h = ctypes.c_void_p()
        rc = lib.st_create_vocoder(ctypes.byref(StVocosConfig(**{**ok, "dim": dim})), 0, ctypes.byref(h))
        assert rc in (ST_OK, ST_ERR_HIP), (dim, rc, lib.st_last_error(None))
        if rc == ST_OK:
            lib.st_destroy(h)
    for dim in (64, 256, 384, 640, 896, 1280):
        h = ctypes.c_void_p()
        assert lib.st_create_vocoder(ctypes.byref(StVocosConfig(**{**ok, "dim": dim})), 0, ctypes.byref(h)) == ST_ERR_UNSUPPORTED, dim
        msg = lib.st_last_error(None).decode()
        assert all(w in msg for w in ("512", "768", "1024")), msg
        assert not h.value
    h = ctypes.c_void_p()
    assert lib.st_create_vocoder(ctypes.byref(StVocosConfig(**{**ok, "dim": 0})), 0, ctypes.byref(h)) == ST_ERR_INVALID
    # the trainer's whole configuration passes the limits too
    rc = lib.st_create_vocoder(ctypes.byref(StVocosConfig(**{**ok, **D.TRAINER})), 0, ctypes.byref(h))
    assert rc in (ST_OK, ST_ERR_HIP), rc
    if rc == ST_OK:
        lib.st_destroy(h)


def test_fixture_is_what_the_generator_says(gold):
    for name, (fields, B, T, *_rest) in D.CASES.items():
        cfg = vo.vocos_config(**fields)
        n = len(gold[name + "/names"])
        assert n == 9 * cfg.num_layers + 8
        assert gold[name + "/dmel64"].shape == (B, cfg.input_channels, T) and gold[name + "/dmel64"].dtype == np.float64
        assert gold[name + "/audio64"].shape == (min(R.FRAMES_SAMPLE, B * T * cfg.hop_length),)
        assert gold[name + "/err32"].shape == gold[name + "/norms"].shape == (n,)
        # the fp32 module's own errors, the GPU test's yardsticks: fp32 rounding, not zero and not large
        for k in ("err32", "dmel_err32", "audio_err32"):
            assert 0 < np.min(gold[f"{name}/{k}"]) and np.max(gold[f"{name}/{k}"]) < 1e-4, (name, k)
    assert D.CASES["trainer"][0] == D.TRAINER == dict(input_channels=128, dim=768, intermediate_dim=2048, num_layers=12)
    assert os.path.getsize(GOLD) < 400 * 1000


@pytest.mark.parametrize("name", list(D.CASES))
def test_oracle_and_restatement_match_the_reference_module(gold, name):
    """The oracle's forward (the GPU inference tests' reference) and the restatement's forward and VJP (the GPU training tests')
    against the real module's float64 audio and gradients at dim 768, 1024 and the trainer's configuration."""
    fields, B, T, wseed, mseed, _ = D.CASES[name]
    cfg = vo.vocos_config(**fields)
    sd, mel = vo.make_vocos_state_dict(wseed, cfg), vo.make_mel(B, T, mseed, M=cfg.input_channels)
    eo = _rel_l2(R.sampled(vo.vocos_forward(sd, mel, cfg), wseed, 1), gold[name + "/audio64"])
    audio, kept = R.forward(sd, mel, cfg)
    assert np.abs(kept["o"][..., :cfg.n_fft // 2 + 1] - np.log(100.0)).min() > 1e-4
    W = R.loss_weights(audio.shape, wseed).astype(np.float64)
    G, dmel = R.backward(sd, kept, W, cfg)
    names = list(gold[name + "/names"])
    assert names == R.param_names(sd) and sorted(G) == names
    l64 = float(gold[name + "/loss64"].reshape(-1)[0])
    lerr = abs(float((audio * W).sum()) - l64) / abs(l64)
    worst = ("", 0.0)
    for i, n in enumerate(names):
        assert G[n].shape == sd[n].shape
        e = _rel_l2(D.stored_elements(name, i, G[n], wseed), gold[f"{name}/grad/{n}"])
        worst = max(worst, (n, e), key=lambda v: v[1])
        assert e <= BAR, (n, e)
        assert abs(np.linalg.norm(G[n]) - gold[name + "/norms"][i]) <= 1e-9 * gold[name + "/norms"][i]
    de, ea = _rel_l2(dmel, gold[name + "/dmel64"]), _rel_l2(R.sampled(audio, wseed, 1), gold[name + "/audio64"])
    print(f"{name}: oracle audio {eo:.1e}, restatement audio {ea:.1e}, loss rel {lerr:.1e}, worst parameter {worst[0]} {worst[1]:.1e}, "
          f"d mel {de:.1e} (bar {BAR:.0e})")
    assert eo <= BAR and ea <= BAR and lerr <= BAR and de <= BAR


@pytest.mark.parametrize("train", [False, True], ids=["vocos", "vocos_train"])
def test_module_at_the_trainers_config_has_the_reference_keys_and_shapes(train):
    """Vocos(VocosConfig(128, 768, 2048, 12), MelConfig()) of vocoders/vocos/train.py:53: the reference's state_dict keys and shapes
    (make_vocos_state_dict writes the reference module's), loaded with strict=True."""
    from stabletts_amd import vocos, vocos_train
    cls = (vocos_train if train else vocos).Vocos
    cfg = vo.vocos_config(**D.TRAINER)
    m = cls(types.SimpleNamespace(**D.TRAINER), types.SimpleNamespace(n_fft=cfg.n_fft, hop_length=cfg.hop_length))
    sd = vo.make_vocos_state_dict(141, cfg)
    have = m.state_dict()
    assert sorted(have) == sorted(sd) and len(have) == 9 * 12 + 9
    for k, v in sd.items():
        assert tuple(have[k].shape) == v.shape, k
    assert have["backbone.convnext.11.pwconv1.weight"].shape == (2048, 768) and have["head.out.weight"].shape == (2050, 768)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert all(p.requires_grad for p in m.parameters()) == train
