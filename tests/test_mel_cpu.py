"""Feature front end without a GPU: the float64 restatement against tests/golden/mel_outputs.npz (tools/make_golden_mel.py), the
drop-in's filter bank and state_dict against the reference module built under the torchaudio stand-in, install(audio=True), the
configuration limits in Python and in st_create_mel_extractor, and the frame-count formula."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests import mel_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mel_outputs.npz")))


def _cases(gold):
    return sorted(k[:-4] for k in gold if k.endswith("/mel"))


def _fb(sr, n_fft, n_mels):
    from stabletts_amd.audio import melscale_fbanks
    return melscale_fbanks(n_fft // 2 + 1, 0.0, float(sr // 2), int(n_mels), int(sr), "slaney", "slaney").numpy()


def test_restatement_reproduces_the_fixture(gold):
    """float64 numpy against the reference's fp32 torch path: within torch's own rounding (the pure tone's floor-level bins
    carry torch's largest fp32 error, 1.4e-3 in the log)."""
    for case in _cases(gold):
        sr, n_fft, hop, pad, n_mels = (int(v) for v in gold[case + "/cfg"])
        wave, win = gold[case + "/wave"], torch.hann_window(n_fft).numpy()
        mel = mr.log_mel(wave, win, _fb(sr, n_fft, n_mels), n_fft, hop, pad)
        lin = mr.linear(wave[:gold[case + "/linear"].shape[0]], win, n_fft, hop, pad)
        assert mel.shape == gold[case + "/mel"].shape, case
        assert np.abs(mel - gold[case + "/mel"]).max() <= (2e-3 if case == "tone" else 1e-4), case
        assert np.abs(lin - gold[case + "/linear"]).max() <= 1e-6 * np.abs(lin).max(), case
    assert np.all(gold["silence/linear"] == np.float32(np.sqrt(np.float32(1e-6))))


def test_fixture_covers_the_issue_cases(gold):
    cases = _cases(gold)
    assert {"default", "silence", "tone", "edge_pad1", "edge_hop", "edge_odd"} <= set(cases)
    assert sorted(int(gold[f"ms{n}/cfg"][1]) for n in (32, 64, 128, 256, 512, 1024, 2048)) == [32, 64, 128, 256, 512, 1024, 2048]
    assert gold["default/wave"].shape[0] == 3 and gold["style_c"].shape == (3, 256)
    pad, hop = 768, 512
    assert gold["edge_pad1/wave"].shape[1] == pad + 1
    assert gold["edge_hop/wave"].shape[1] % hop == 0 and gold["edge_odd/wave"].shape[1] % hop != 0


def test_dropin_filter_bank_and_state_dict_equal_the_reference_module(gold):
    """The fixture records the reference module's state_dict ("name:shape") and the SHA-256 of its fb bytes, built under the
    torchaudio stand-in of tools/make_golden_mel.py: the drop-in has the same keys and shapes and builds the same bank."""
    import hashlib
    from stabletts_amd import audio
    for case in _cases(gold):
        sr, n_fft, hop, pad, n_mels = (int(v) for v in gold[case + "/cfg"])
        m = audio.LogMelSpectrogram(sr, n_fft, n_fft, hop, 0.0, None, pad, n_mels, False, "reflect", "slaney")
        sd = m.state_dict()
        assert [f"{k}:{'x'.join(map(str, v.shape))}" for k, v in sd.items()] == list(gold[case + "/state_dict"]), case
        assert hashlib.sha256(sd["mel_scale.fb"].numpy().tobytes()).hexdigest() == str(np.asarray(gold[case + "/fb_sha256"]).reshape(-1)[0]), case
        assert torch.equal(sd["spectrogram.window"], torch.hann_window(n_fft))
    lin = audio.LinearSpectrogram(2048, 2048, 512, 768, False, "reflect")
    assert [f"{k}:{'x'.join(map(str, v.shape))}" for k, v in lin.state_dict().items()] == list(gold["linear_state_dict"])


def test_filter_bank_formula_htk_and_unnormalised():
    """melscale_fbanks, htk scale without norm: triangles of height at most 1, none empty; f_max=None is sample_rate // 2;
    unknown norm / scale names raise as torchaudio does."""
    from stabletts_amd.audio import melscale_fbanks, MelScale
    fb = melscale_fbanks(513, 0.0, 8000.0, 40, 16000, None, "htk").numpy()
    assert fb.shape == (513, 40) and fb.min() >= 0 and fb.max() <= 1.0 and (fb.max(0) > 0.5).all()
    m = MelScale(40, 16000, 0.0, None, 513, None, "htk")       # f_max None -> sample_rate // 2
    assert np.array_equal(m.fb.numpy(), fb)
    with pytest.raises(ValueError):
        melscale_fbanks(513, 0.0, 8000.0, 40, 16000, "area", "htk")
    with pytest.raises(ValueError):
        melscale_fbanks(513, 0.0, 8000.0, 40, 16000, None, "bark")


def test_install_registers_the_audio_module():
    import stabletts_amd
    from stabletts_amd import audio
    saved = sys.modules.get("utils.audio")
    try:
        stabletts_amd.install(audio=True)
        from utils.audio import LogMelSpectrogram, LinearSpectrogram, load_and_resample_audio      # api.py:17, preprocess.py:11
        assert LogMelSpectrogram is audio.LogMelSpectrogram and LinearSpectrogram is audio.LinearSpectrogram
        assert load_and_resample_audio is audio.load_and_resample_audio
    finally:
        if saved is None:
            sys.modules.pop("utils.audio", None)
        else:
            sys.modules["utils.audio"] = saved


def test_default_install_leaves_utils_audio_alone():
    import stabletts_amd
    saved = sys.modules.pop("utils.audio", None)
    try:
        stabletts_amd.install()
        assert "utils.audio" not in sys.modules
    finally:
        if saved is not None:
            sys.modules["utils.audio"] = saved


def test_mel_config_default_constructs():
    from stabletts_amd.audio import LogMelSpectrogram
    kw = dict(sample_rate=44100, n_fft=2048, win_length=2048, hop_length=512, f_min=0.0, f_max=None, pad=768, n_mels=128,
              center=False, pad_mode="reflect", mel_scale="slaney")
    m = LogMelSpectrogram(**kw)
    assert m.n_mels == 128 and m.mel_scale.fb.shape == (1025, 128) and m.spectrogram.window.shape == (2048,)
    x = torch.log(torch.clamp(torch.tensor([0.0, 1e-6, 2.0]), min=1e-5))
    assert torch.equal(m.compress(torch.tensor([0.0, 1e-6, 2.0])), x) and torch.equal(m.decompress(x), torch.exp(x))


BAD = [  # (overrides of the default config, Python exception, C code)
    (dict(center=True), NotImplementedError, "UNSUPPORTED"),
    (dict(pad_mode="constant"), NotImplementedError, "UNSUPPORTED"),
    (dict(pad_mode="replicate"), NotImplementedError, "UNSUPPORTED"),
    (dict(win_length=1024), NotImplementedError, "UNSUPPORTED"),
    (dict(n_fft=1000, win_length=1000, hop_length=250), NotImplementedError, "UNSUPPORTED"),
    (dict(n_fft=16, win_length=16, hop_length=4), NotImplementedError, "UNSUPPORTED"),
    (dict(n_fft=4096, win_length=4096), NotImplementedError, "UNSUPPORTED"),
    (dict(hop_length=0), ValueError, "INVALID"),
    (dict(hop_length=4096), ValueError, "INVALID"),
    (dict(pad=-1), ValueError, "INVALID"),
    (dict(n_fft=0, win_length=0), ValueError, "INVALID"),
]


@pytest.mark.parametrize("over,exc,code", BAD)
def test_unsupported_and_invalid_configs_raise(over, exc, code):
    from stabletts_amd import _lib
    from stabletts_amd.audio import LogMelSpectrogram
    kw = dict(sample_rate=44100, n_fft=2048, win_length=2048, hop_length=512, f_min=0.0, f_max=None, pad=768, n_mels=128,
              center=False, pad_mode="reflect", mel_scale="slaney")
    kw.update(over)
    with pytest.raises(exc):
        LogMelSpectrogram(**kw)
    lib = _lib.load()
    cfg = _lib.StMelConfig(kw["n_fft"], kw["win_length"], kw["hop_length"], kw["pad"], kw["n_mels"], int(kw["center"]),
                           _lib.ST_PAD_MODES[kw["pad_mode"]])
    h = ctypes.c_void_p()
    want = _lib.ST_ERR_UNSUPPORTED if code == "UNSUPPORTED" else _lib.ST_ERR_INVALID
    assert lib.st_create_mel_extractor(ctypes.byref(cfg), 0, ctypes.byref(h)) == want, over
    assert lib.st_last_error(None)


def test_c_abi_rejects_bad_configs_and_foreign_handles_without_a_gpu():
    from stabletts_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    for over, code in ((dict(n_mels=-1), _lib.ST_ERR_INVALID), (dict(pad_mode=9), _lib.ST_ERR_INVALID),
                       (dict(hop_length=-3), _lib.ST_ERR_INVALID)):
        base = dict(n_fft=2048, win_length=2048, hop_length=512, pad=768, n_mels=128, center=0, pad_mode=0)
        base.update(over)
        assert lib.st_create_mel_extractor(ctypes.byref(_lib.StMelConfig(**base)), 0, ctypes.byref(h)) == code, over
    assert lib.st_create_mel_extractor(None, 0, ctypes.byref(h)) == _lib.ST_ERR_INVALID
    assert lib.st_mel_frames(None, 10000) == _lib.ST_ERR_INVALID
    assert lib.st_mel_forward(None, None, 1, 10000, None, None) == _lib.ST_ERR_INVALID


@pytest.mark.parametrize("n_fft", [32, 64, 128, 256, 512, 1024, 2048])
def test_frame_count_formula(n_fft):
    from stabletts_amd.audio import frames
    hop, pad = n_fft // 4, (n_fft - n_fft // 4) // 2
    for L in (pad + 1, 2 * n_fft, 6 * hop, 6 * hop + 1, 6 * hop + hop - 1, 44100):
        if L + 2 * pad < n_fft:
            continue
        T = frames(L, n_fft, hop, pad)
        assert T == mr.frames(L, n_fft, hop, pad) == len(range(0, L + 2 * pad - n_fft + 1, hop))
        assert (T - 1) * hop + n_fft <= L + 2 * pad < T * hop + n_fft
    with pytest.raises(ValueError):
        frames(pad, n_fft, hop, pad)         # reflect padding needs pad < L
    assert frames(pad + 1, n_fft, hop, pad) == 1 + (3 * pad + 1 - n_fft) // hop if 3 * pad + 1 >= n_fft else True


def test_frame_count_matches_the_fixture(gold):
    from stabletts_amd.audio import frames
    for case in _cases(gold):
        _, n_fft, hop, pad, _ = (int(v) for v in gold[case + "/cfg"])
        assert gold[case + "/mel"].shape[2] == frames(gold[case + "/wave"].shape[1], n_fft, hop, pad), case
    assert frames(769, 2048, 512, 768) == 1
    with pytest.raises(ValueError):
        frames(100, 2048, 512, 768)
    with pytest.raises(ValueError):
        frames(40, 2048, 512, 8)             # L + 2 pad < n_fft: torch.stft has no frame


def test_cpu_module_raises_instead_of_falling_back():
    from stabletts_amd.audio import LogMelSpectrogram, load_and_resample_audio
    m = LogMelSpectrogram(44100, 2048, 2048, 512, 0.0, None, 768, 128, False, "reflect", "slaney")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 4096))
    try:
        import torchaudio  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="torchaudio"):
            load_and_resample_audio("missing.wav", 44100)
