"""The training side of the alignment step on a CPU-only box: the float64 restatement (tests/align_loss_restatement.py)
reproduces the losses and gradients that the REAL reference StableTTS.forward gave in float64 (tests/golden/align_loss_grads.npz,
tools/make_golden_align_losses.py); the library exports the new entry points, which reject bad arguments on the host;
stabletts_amd.model.StableTTS has the reference's checkpoint layout; install(model=True) registers it and nothing else."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import align_loss_restatement as ar
from tests.align_loss_restatement import CASES, GOLDEN, case_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = os.path.join(ROOT, "tests", "golden", "stabletts_layout.npz")
SYMBOLS = ("st_align_train_forward", "st_align_train_backward", "st_align_train_scratch_floats", "st_duration_loss",
           "st_duration_loss_backward", "st_duration_loss_scratch_floats")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def test_fixture_cases_are_what_they_claim(gold):
    assert {k.split("/")[0] for k in gold} == set(CASES)
    g = case_of(gold, "ragged")
    assert g["mu_x"].shape == (4, 80, 37) and g["y"].shape == (4, 80, 300)
    assert g["x_lengths"][0] == 37 and g["y_lengths"][0] == 300 and len(set(g["x_lengths"])) == 4
    assert g["durations"].max() == 270 and (g["durations"] == 1).sum() >= 10
    assert g["keep"].any() and not g["keep"].all()
    g = case_of(gold, "wide")
    assert g["mu_x"].shape[:2] == (3, 100) and g["x_lengths"][0] > g["y_lengths"][0]
    assert (g["durations"][0, :g["x_lengths"][0]] == 0).any() and g["keep"].any() and not g["keep"].all()
    d, k = case_of(gold, "edges_dropped"), case_of(gold, "edges_kept")
    assert not d["keep"].any() and k["keep"].all()
    assert d["x_lengths"][0] == 1 and d["y_lengths"][1] == 1
    assert d["x_lengths"][2] == d["mu_x"].shape[2] and d["y_lengths"][2] == d["y"].shape[2]
    for key in ("mu_x", "logw", "y", "W", "fake_content", "durations"):
        assert np.array_equal(d[key], k[key])
    for name in CASES:
        g = case_of(gold, name)
        assert (g["durations"].sum(1) == g["y_lengths"]).all()
        assert np.abs(g["fake_content"]).min() > 0


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_float64_reference(gold, case):
    g = case_of(gold, case)
    f = ar.forward(g["mu_x64"], g["x_mask"], g["logw64"], g["x_lengths"], g["y64"], g["y_mask"], g["durations"], g["keep"],
                   g["fake_content64"])
    assert abs(f["prior_loss"] - g["prior_loss_f64"]) <= 1e-12 * abs(g["prior_loss_f64"])
    assert abs(f["dur_loss"] - g["dur_loss_f64"]) <= 1e-12 * abs(g["dur_loss_f64"])
    assert abs(np.sum(g["W64"] * f["mu_y_masked"]) - g["diff_loss_f64"]) <= 1e-12 * np.sum(np.abs(g["W64"] * f["mu_y_masked"]))
    assert np.array_equal(f["mu_y"].astype(np.float32), g["mu_y"])                  # a gather: exact
    assert np.array_equal(f["mu_y_masked"].astype(np.float32), g["mu_y_masked"])
    r = ar.backward(g["mu_x64"], g["x_mask"], g["logw64"], g["x_lengths"], g["y64"], g["y_mask"], g["durations"], g["keep"],
                    g_masked=g["W64"], g_prior=1.0, g_dur=1.0)
    assert rel(r["grad_mu_x"], g["grad_mu_x_f64"]) <= 1e-12
    assert rel(r["grad_logw"], g["grad_logw_f64"]) <= 1e-12
    if g["keep"].all():
        assert not g["grad_fake_content_f64"].any() and not r["grad_fake_content"].any()
    else:
        assert rel(r["grad_fake_content"], g["grad_fake_content_f64"].reshape(-1)) <= 1e-12
    # a token without frames has no term, and its gradient is exactly 0 in the reference too
    assert not g["grad_mu_x_f64"].transpose(0, 2, 1)[r["n"] == 0].any() and not r["S"].transpose(0, 2, 1)[r["n"] == 0].any()


@pytest.mark.parametrize("case", CASES)
def test_frame_token_is_the_column_of_the_reference_alignment(gold, case):
    g = case_of(gold, case)
    attn = g["attn"]                                                                # (B, Tx, Ty) 0/1
    tok = ar.frame_token(g["durations"], g["x_mask"], attn.shape[2])
    assert attn.sum(1).max() == 1
    want = np.where(attn.sum(1) == 1, attn.argmax(1), -1)
    assert tok.dtype == np.int32 and np.array_equal(tok, want)


def test_restatement_clips_malformed_durations():
    dur = np.array([[5, -3, 9, 4], [2, 2, 2, 7]])
    x_mask = np.array([[1, 1, 1, 1], [1, 1, 1, 0]], np.float32)
    assert np.array_equal(ar.segment_ends(dur, x_mask, 10), [[5, 5, 10, 10], [2, 4, 6, 6]])
    tok = ar.frame_token(dur, x_mask, 10)
    assert np.array_equal(tok[0], [0] * 5 + [2] * 5) and np.array_equal(tok[1], [0, 0, 1, 1, 2, 2, -1, -1, -1, -1])
    assert np.array_equal(ar.segment_ends(np.array([[2 ** 31 - 1, 2 ** 31 - 1]]), np.ones((1, 2)), 7), [[7, 7]])


@pytest.fixture(scope="module")
def lib():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    return _lib.load()


def test_symbols_are_exported_and_the_abi_is_unchanged(lib):
    from stabletts_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.st_abi_version() == 4
    assert lib.st_duration_loss_scratch_floats() >= 2
    # one partial pair per block of 256 frames x 16 channels, then the sum and the denominator
    assert lib.st_align_train_scratch_floats(64, 80, 1000) == 2 * 4 * 5 * 64 + 2
    assert lib.st_align_train_scratch_floats(1, 1, 1) == 4
    assert lib.st_align_train_scratch_floats(0, 80, 10) == _lib.ST_ERR_INVALID


def test_entry_points_reject_on_the_host(lib):
    from stabletts_amd import _lib
    p = ctypes.c_void_p(16)              # never dereferenced: every call below returns before any launch
    fwd = lambda *shape, dur=p, out=p: lib.st_align_train_forward(dur, p, p, p, p, None, None, *shape, p, None, out, p, p, None)   # noqa: E731
    assert fwd(1, 80, 4, 4, dur=None) == _lib.ST_ERR_INVALID and fwd(1, 80, 4, 4, out=None) == _lib.ST_ERR_INVALID
    assert fwd(0, 80, 4, 4) == _lib.ST_ERR_INVALID and fwd(1, 80, 0, 4) == _lib.ST_ERR_INVALID
    assert fwd(1, 80, 4097, 4) == _lib.ST_ERR_UNSUPPORTED and "4096" in lib.st_last_error(None).decode()
    bwd = lambda *shape, gp=None, y=p, out=p: lib.st_align_train_backward(p, p, p, p, y, None, p, p, None, gp, *shape, out, None, None)   # noqa: E731
    assert bwd(1, 80, 4, 4, out=None) == _lib.ST_ERR_INVALID and bwd(1, 80, 4, 0) == _lib.ST_ERR_INVALID
    assert bwd(1, 80, 4, 4, gp=p, y=None) == _lib.ST_ERR_INVALID and "grad_prior" in lib.st_last_error(None).decode()
    assert bwd(1, 80, 4097, 4) == _lib.ST_ERR_UNSUPPORTED
    assert lib.st_duration_loss(None, p, p, p, 1, 4, None, p, p, None) == _lib.ST_ERR_INVALID
    assert lib.st_duration_loss(p, p, p, p, 1, 0, None, p, p, None) == _lib.ST_ERR_INVALID
    assert lib.st_duration_loss_backward(p, p, p, p, None, 1, 4, p, None) == _lib.ST_ERR_INVALID


def test_align_and_losses_has_no_cpu_fallback():
    import torch
    from stabletts_amd.alignment import align_and_losses
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align_and_losses(torch.zeros(1, 2, 3), torch.ones(1, 1, 3), torch.zeros(1, 1, 3), torch.tensor([3]), torch.zeros(1, 2, 4),
                         torch.ones(1, 1, 4), torch.tensor([[1, 1, 2]]))


def test_dense_alignment_from_frame_tokens(gold):
    import torch
    from stabletts_amd.alignment import dense_alignment
    for case in CASES:
        g = case_of(gold, case)
        tok = torch.from_numpy(ar.frame_token(g["durations"], g["x_mask"], g["y"].shape[2]))
        attn = dense_alignment(tok, g["mu_x"].shape[2])
        assert attn.dtype == torch.float32 and np.array_equal(attn.numpy(), g["attn"].astype(np.float32))


def test_native_stabletts_has_the_reference_layout():
    import torch
    from stabletts_amd.model import StableTTS, generate_path       # noqa: F401  (models.model exports both)
    g = np.load(LAYOUT)
    args = [int(v) if float(v).is_integer() else float(v) for v in g["model_args"].tolist()]
    model = StableTTS(*args)
    sd = model.state_dict()
    assert list(sd.keys()) == g["state_dict.names"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g["state_dict.shapes"].tolist()
    assert (model.n_vocab, model.mel_channels, model.cfg_dropout) == (args[0], args[1], 0.2)
    assert isinstance(model.fake_speaker, torch.nn.Parameter) and model.fake_speaker.shape == (1, args[9])
    assert isinstance(model.fake_content, torch.nn.Parameter) and model.fake_content.shape == (1, args[1], 1)
    assert not model.fake_speaker.any() and not model.fake_content.any() and model.return_attn is True
    assert model.decoder.sigma_min == float(g["decoder.sigma_min"])
    assert model.ref_encoder.native_training and model.dp.native_training
    assert all(type(m).__module__.startswith("stabletts_amd.") for m in (model.encoder, model.ref_encoder, model.dp, model.decoder))
    with pytest.raises(RuntimeError):                                # no CPU fallback: the first submodule refuses
        model(torch.zeros(1, 4, dtype=torch.long), torch.tensor([4]), torch.zeros(1, args[1], 8), torch.tensor([8]),
              torch.zeros(1, args[1], 8), torch.tensor([8]))


@pytest.mark.parametrize("others", [dict(), dict(text_encoder=True, reference_encoder="train", duration_predictor="train",
                                                  monotonic_align=True)])
def test_install_registers_models_model_and_nothing_else(others):
    import stabletts_amd
    watched = ("models.model", "models.flow_matching", "models.text_encoder", "models.reference_encoder", "models.duration_predictor",
               "monotonic_align", "utils.audio", "vocoders.vocos.models.model")
    saved = {k: sys.modules.get(k) for k in watched}

    def snapshot(**kw):
        for k in watched:
            sys.modules.pop(k, None)
        stabletts_amd.install(**kw)
        return {k: v for k, v in sys.modules.items() if not k.startswith("stabletts_amd")}

    try:
        without = snapshot(**others)
        assert "models.model" not in without
        with_model = snapshot(model=True, **others)
        md = with_model.pop("models.model")
        assert md.__name__ == "stabletts_amd.model" and md.StableTTS is stabletts_amd.StableTTS and callable(md.generate_path)
        assert with_model.keys() == without.keys() and all(with_model[k] is without[k] for k in without)
        from models.model import StableTTS                          # train.py:18
        assert StableTTS is md.StableTTS
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m
