"""CPU checks of the Vocos vocoder at n_fft 256-1024 (hop_length n_fft / 4) and mel widths in steps of 16: the creation limits of
st_create_vocoder, the float64 oracle's forward pinned to the REAL reference module at three such configurations
(tests/golden/vocos_rates.npz, tools/make_golden_vocos_rates.py), and the switch points of the head GEMM's tiles that
tests/test_gpu_vocos_rates.py straddles."""
import ctypes
import os

import numpy as np
import pytest

from oracle import vocos_oracle as vo
from tests import vocos_rates_cases as D
from tests.test_gpu_vocos_shapes import tile_of
from tests.test_vocos_dims_cpu import BAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vocos_rates.npz")


@pytest.fixture(scope="module")
def lib():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    return _lib.load()


def _create(lib, **fields):
    from stabletts_amd._lib import StVocosConfig
    cfg = dict(input_channels=128, dim=512, intermediate_dim=1536, num_layers=8, n_fft=2048, hop_length=512, operand_dtype=0)
    h = ctypes.c_void_p()
    rc = lib.st_create_vocoder(ctypes.byref(StVocosConfig(**{**cfg, **fields})), 0, ctypes.byref(h))
    return rc, h


def test_creation_accepts_the_four_n_fft_and_mel_widths_in_steps_of_16(lib):
    """Every (n_fft, n_fft / 4, M) with n_fft in {256, 512, 1024, 2048} and M a multiple of 16 up to 192 passes the limits at dim 512,
    and (1024, 256, 80) at dim 768 and 1024 (on a box without a GPU creation then ends in ST_ERR_HIP, with one in ST_OK)."""
    from stabletts_amd._lib import ST_ERR_HIP, ST_OK
    cases = [dict(n_fft=n, hop_length=n // 4, input_channels=m) for n in D.N_FFTS for m in D.MEL_WIDTHS]
    cases += [dict(n_fft=1024, hop_length=256, input_channels=80, dim=dim) for dim in (768, 1024)]
    assert len(cases) == 4 * 12 + 2
    for fields in cases:
        rc, h = _create(lib, **fields)
        assert rc in (ST_OK, ST_ERR_HIP), (fields, rc, lib.st_last_error(None))
        if rc == ST_OK:
            lib.st_destroy(h)


@pytest.mark.parametrize("fields,words", [
    (dict(n_fft=128, hop_length=32), ("256", "512", "1024", "2048", "hop_length == n_fft / 4")),
    (dict(n_fft=1000, hop_length=250), ("256", "512", "1024", "2048", "hop_length == n_fft / 4")),
    (dict(n_fft=4096, hop_length=1024), ("256", "512", "1024", "2048", "hop_length == n_fft / 4")),
    (dict(n_fft=1024, hop_length=512), ("hop_length == n_fft / 4",)),
    (dict(n_fft=2048, hop_length=256), ("hop_length == n_fft / 4",)),
    (dict(n_fft=1024, hop_length=128), ("hop_length == n_fft / 4",)),
    (dict(n_fft=512, hop_length=512), ("hop_length == n_fft / 4",)),
    (dict(input_channels=8), ("multiple of 16 up to 192",)),
    (dict(input_channels=100), ("multiple of 16 up to 192",)),
    (dict(input_channels=200), ("multiple of 16 up to 192",)),
    (dict(input_channels=208), ("multiple of 16 up to 192",)),
], ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else "")
def test_creation_refuses_everything_else_and_names_the_rule(lib, fields, words):
    """ST_ERR_UNSUPPORTED with a null handle, before a device is touched, and a message that states the rule."""
    from stabletts_amd._lib import ST_ERR_UNSUPPORTED
    rc, h = _create(lib, **fields)
    msg = lib.st_last_error(None).decode()
    assert rc == ST_ERR_UNSUPPORTED, (fields, rc, msg)
    assert not h.value
    assert all(w in msg for w in words), msg


def test_fixture_is_what_the_generator_says():
    gold = np.load(GOLD)
    assert sorted(gold.files) == sorted(name + "/audio64" for name in D.CASES)
    for name, (fields, B, T, _, _) in D.CASES.items():
        cfg = vo.vocos_config(**fields)
        assert cfg.hop_length * 4 == cfg.n_fft and cfg.input_channels % 64 != 0
        a = gold[name + "/audio64"]
        assert a.shape == (B, T * cfg.hop_length) and a.dtype == np.float64
        assert np.isfinite(a).all() and np.abs(a).max() > 1e-2
    assert [(vo.vocos_config(**f).n_fft, vo.vocos_config(**f).input_channels, vo.vocos_config(**f).dim) for f, *_ in D.CASES.values()] == \
        [(1024, 80, 512), (512, 96, 768), (256, 16, 1024)]
    assert os.path.getsize(GOLD) < 400 * 1000


@pytest.mark.parametrize("name", list(D.CASES))
def test_oracle_matches_the_reference_module(name):
    """The oracle's forward (the reference of tests/test_gpu_vocos_rates.py) against the real module's float64 audio."""
    fields, B, T, wseed, mseed = D.CASES[name]
    cfg = vo.vocos_config(**fields)
    ref = np.load(GOLD)[name + "/audio64"]
    got = vo.vocos_forward(vo.make_vocos_state_dict(wseed, cfg), vo.make_mel(B, T, mseed, M=cfg.input_channels), cfg)
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print(f"{name}: oracle audio rel L2 {err:.1e} (bar {BAR:.0e})")
    assert got.shape == ref.shape and err <= BAR


def test_head_tile_switch_points():
    """The head GEMM's cout is 2 * round_up(n_fft / 2 + 1, 128): 1280, 768 and 512 at n_fft 1024, 512 and 256.  Where gemm() changes
    its tile for them (tile_of restates engine.cpp), which the GPU test's batches straddle."""
    def first(pred, stop=40000):
        return next((R for R in range(1, stop) if pred(R)), None)
    assert [2 * ((n // 2 + 1 + 127) // 128 * 128) for n in (1024, 512, 256, 2048)] == [1280, 768, 512, 2304]
    assert first(lambda R: tile_of(R, 1280, "F32") != "T64") == 3201
    assert first(lambda R: tile_of(R, 1280, "F32") == "BIG") == 9729
    assert first(lambda R: tile_of(R, 768, "F32") != "T64") == 5377
    # cout 768 and 512 take BIG tiles only beyond the ~10 k rows a quick test can afford (3 and 2 column tiles need 64 and 96 row tiles)
    assert first(lambda R: tile_of(R, 768, "F32") == "BIG") == 16129
    assert first(lambda R: tile_of(R, 512, "F32") != "T64") == 8193
    assert first(lambda R: tile_of(R, 512, "F32") == "BIG") == 24321
