"""The spectrogram's backward without a GPU: the float64 restatement tests/mel_vjp_restatement.py (steps 1-5 of st_mel_backward)
against torch.autograd in float64 on every configuration of tests/golden/mel_outputs.npz, the index inversion of step 5 against a
brute-force scatter at the padding edges and off the hop = n_fft / 4 lattice (tests/mel_checks.py), install(audio="train"), and the new C entry points on a null handle."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import mel_checks as mc
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


@pytest.mark.parametrize("n_fft,hop,pad,T,L", mc.GEOMETRIES, ids=lambda v: str(v))
def test_gather_by_index_inversion_equals_a_scatter_off_the_lattice(n_fft, hop, pad, T, L):
    """The same off the hop = n_fft / 4 lattice: every (n_fft, hop, pad) and L of tests/mel_checks.py (hop 1, hop = n_fft, odd hops,
    pad 0, pad > hop, pad = n_fft - 1, an unread tail).  Measured: at most 3.1e-16 relative."""
    frames = mr.frames(L, n_fft, hop, pad)
    assert frames == T
    rng = np.random.Generator(np.random.PCG64(n_fft + 7 * hop + 11 * pad + L))
    wdf = rng.standard_normal((2, frames, n_fft))
    a, b = mv.gather(wdf, L, hop, pad), mv.scatter(wdf, L, hop, pad)
    assert a.shape == (2, L) and np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (n_fft, hop, pad, L)


@pytest.mark.parametrize("n_fft,hop,pad,T,L", mc.GEOMETRIES, ids=lambda v: str(v))
def test_restatement_equals_torch_autograd_off_the_lattice(n_fft, hop, pad, T, L):
    """mv.vjp against torch float64 autograd of mv.torch_forward at the geometries of tests/mel_checks.py with the asymmetric window
    (uniform(0.5, 1.5): non-zero ends, w[n] != w[N - 1 - n]), log-mel and linear.  Measured: at most 3.7e-14; bar 1e-10."""
    n_mels = min(m for (n, h, p, m) in mc.CONFIGS if (n, h, p) == (n_fft, hop, pad))
    wave = mc.waves(2, L, n_fft + hop + pad + L).astype(np.float64)
    win = torch.from_numpy(mc.window(n_fft).astype(np.float64))
    fb = torch.from_numpy(mc.slaney(n_fft, n_mels).astype(np.float64))
    rng = np.random.Generator(np.random.PCG64(L))
    for bank in (fb, None):
        x = torch.from_numpy(wave).requires_grad_(True)
        y = mv.torch_forward(x, win, bank, n_fft, hop, pad)
        g = rng.standard_normal(tuple(y.shape))
        (dx,) = torch.autograd.grad(y, x, torch.from_numpy(g))
        ref = dx.numpy()
        with np.errstate(divide="ignore", invalid="ignore"):                     # an empty filter: g / 0 under the mask
            got = mv.vjp(wave, win.numpy(), None if bank is None else bank.numpy(), n_fft, hop, pad, g)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"{(n_fft, hop, pad)} T={T} L={L} {'log-mel' if bank is not None else 'linear'}: restatement vs torch float64 {err:.2e} (bar 1e-10)")
        assert y.shape[-1] == T and got.shape == ref.shape == (2, L) and err <= 1e-10


def test_sweep_geometries_reach_what_they_are_for():
    """The case table itself: the frame counts around the FFT round and the block, the lengths, and each configuration's reason."""
    assert len(mc.CONFIGS) == 9 and {c[0] for c in mc.HANN_CONFIGS} == {32, 64, 128, 256, 512, 1024, 2048}
    for cfg in mc.CONFIGS:
        n_fft, hop, pad, n_mels = cfg
        S, FR = mc.tile(n_fft)
        counts = mc.frame_counts(cfg)
        Ts = [T for T, _ in counts]
        assert all(mr.frames(L, n_fft, hop, pad) == T and mr.frames(L + 1, n_fft, hop, pad) in (T, T + 1) and L > pad for T, L in counts)
        least = mr.frames(max(pad + 1, n_fft - 2 * pad), n_fft, hop, pad)         # the smallest the configuration allows
        want = {T for T in (S + 1, FR + 1, 2 * FR + 1) if least <= T <= mc.T_LIMIT.get(cfg, T)}
        assert want <= set(Ts) and min(Ts) == least, cfg
        for T, L in counts:                                                       # the largest L of that T, unless raised
            assert mr.frames(L + 1, n_fft, hop, pad) == T + 1 or L == max(pad + 1, n_fft - 2 * pad), (cfg, T, L)
    empty = lambda n, m: int((mc.slaney(n, m) != 0).any(0).__invert__().sum())
    assert empty(32, 64) == 39 and empty(2048, 4096) == 2385 and empty(32, 5) == 0 and empty(512, 80) == 0
    T, L = mc.frame_counts((128, 100, 3, 20))[-1]
    assert L - 1 - ((T - 1) * 100 + 127 - 3) == 96                              # samples past the last frame's last read
    assert mc.frame_counts((256, 64, 255, 40))[0][1] == 256                     # L = pad + 1
    # sample 5 there: padded position 260 (frames 1-4) and its left reflection 250 (frames 0-3)
    assert mc.readers(5, 256, 8, 256, 64, 255).tolist() == [0, 1, 2, 3, 4]


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
