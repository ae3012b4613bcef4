"""The spectrogram's backward without a GPU: the float64 restatement tests/mel_vjp_restatement.py (steps 1-5 of st_mel_backward)
against torch.autograd in float64 on every configuration of tests/golden/mel_outputs.npz, the index inversion of step 5 against a
brute-force scatter at the padding edges, install(audio="train"), and the new C entry points on a null handle."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import mel_restatement as mr
from tests import mel_vjp_restatement as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["default", "silence", "tone", "edge_pad1", "edge_hop", "edge_odd"] + [f"ms{n}" for n in (32, 64, 128, 256, 512, 1024, 2048)]
UTILS_AUDIO_NAMES = ("LinearSpectrogram", "LogMelSpectrogram", "load_and_resample_audio")      # utils/audio.py's definitions


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mel_outputs.npz")))


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_torch_autograd_in_float64(gold, case):
    from stabletts_amd.audio import melscale_fbanks
    sr, n_fft, hop, pad, n_mels = (int(v) for v in gold[case + "/cfg"])
    wave = gold[case + "/wave"]
    win = torch.hann_window(n_fft, dtype=torch.float64)
    fb = melscale_fbanks(n_fft // 2 + 1, 0.0, float(sr // 2), n_mels, sr, "slaney", "slaney").double()
    rng = np.random.Generator(np.random.PCG64(int.from_bytes(case.encode(), "little") % (1 << 32)))
    for bank in (fb, None):
        x = torch.from_numpy(wave).double().requires_grad_(True)
        y = mv.torch_forward(x, win, bank, n_fft, hop, pad)
        g = rng.standard_normal(tuple(y.shape))
        (dx,) = torch.autograd.grad(y, x, torch.from_numpy(g))
        ref = dx.numpy()
        got = mv.vjp(wave, win.numpy(), None if bank is None else bank.numpy(), n_fft, hop, pad, g)
        err = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))      # silence: both exactly 0
        print(f"{case} {'log-mel' if bank is not None else 'linear'}: restatement vs torch float64 {err:.2e} (gate 1e-10)")
        assert got.shape == ref.shape and err <= 1e-10


@pytest.mark.parametrize("n_fft", [32, 256, 2048])
def test_gather_by_index_inversion_equals_a_scatter(n_fft):
    hop, pad = n_fft // 4, (n_fft - n_fft // 4) // 2
    rng = np.random.Generator(np.random.PCG64(n_fft))
    for L in (pad + 1, pad + 2, 7 * hop, 7 * hop + 3, max(n_fft - 2 * pad, pad + 1)):
        T = mr.frames(L, n_fft, hop, pad)
        wdf = rng.standard_normal((2, T, n_fft))
        a, b = mv.gather(wdf, L, hop, pad), mv.scatter(wdf, L, hop, pad)
        assert a.shape == (2, L) and np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (n_fft, L)


def test_install_audio_train_registers_trainable_spectrograms():
    import stabletts_amd
    from stabletts_amd import audio
    saved = sys.modules.get("utils.audio")
    try:
        stabletts_amd.install(audio="train")
        ua = importlib.import_module("utils.audio")
        from stabletts_amd import audio_train
        assert ua is audio_train
        for name in UTILS_AUDIO_NAMES:
            assert hasattr(ua, name), name
        assert ua.LogMelSpectrogram.native_training is True and ua.LinearSpectrogram.native_training is True
        assert issubclass(ua.LogMelSpectrogram, audio.LogMelSpectrogram) and issubclass(ua.LinearSpectrogram, audio.LinearSpectrogram)
        assert ua.load_and_resample_audio is audio.load_and_resample_audio
        assert audio.LogMelSpectrogram.native_training is False and audio.LinearSpectrogram.native_training is False
        m = ua.LogMelSpectrogram(44100, 32, 32, 8, 0.0, None, 12, 5, False, "reflect", "slaney")
        assert list(m.state_dict()) == list(audio.LogMelSpectrogram(44100, 32, 32, 8, 0.0, None, 12, 5, False, "reflect",
                                                                    "slaney").state_dict())
        stabletts_amd.install(audio=True)
        assert importlib.import_module("utils.audio") is audio
    finally:
        if saved is None:
            sys.modules.pop("utils.audio", None)
        else:
            sys.modules["utils.audio"] = saved


def test_backward_entry_points_reject_a_null_handle():
    from stabletts_amd import _lib
    lib = _lib.load()
    assert "st_mel_backward" in _lib.EXPORTS and "st_mel_backward_workspace_bytes" in _lib.EXPORTS
    assert lib.st_mel_backward(None, None, None, 1, 10000, _lib.ST_MEL_LOG, None, None, None) == _lib.ST_ERR_INVALID
    assert lib.st_mel_backward_workspace_bytes(None, 1, 10000) == _lib.ST_ERR_INVALID


def test_trainable_module_on_cpu_raises_instead_of_falling_back():
    from stabletts_amd.audio_train import LogMelSpectrogram
    m = LogMelSpectrogram(44100, 32, 32, 8, 0.0, None, 12, 5, False, "reflect", "slaney")
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 100, requires_grad=True))
