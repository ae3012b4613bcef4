"""Native feature front end (audio_kernels.hip) on a real MI355X: every case of tests/golden/mel_outputs.npz (the reference's
utils/audio.py run by tools/make_golden_mel.py) and the float64 restatement tests/mel_restatement.py, for the log-mel and the
linear spectrogram; ragged batches, repeatability, loaded buffers, the api.py chain into the native MelStyleEncoder, the C ABI.

Gates: log-mel max abs error <= 1e-3 against the fixture and against float64; linear magnitude max|d| / max|ref| <= 1e-5 against
float64.  Each case prints the reference's own fp32 error against float64 beside the native one.  The pure tone is the exception:
there torch's fp32 path itself misses 1e-3 against float64 (1.4e-3, on floor-level bins next to the tone), so that case is gated
relative to torch's error instead: native vs float64 <= 2 x torch's error, native vs fixture <= 3 x torch's error.
Run with ``-m gpu``."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import mel_restatement as mr
from tests import synth_weights as sw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mel_outputs.npz")))


CASES = ["default", "silence", "tone", "edge_pad1", "edge_hop", "edge_odd"] + [f"ms{n}" for n in (32, 64, 128, 256, 512, 1024, 2048)]


def _modules(gold, case):
    from stabletts_amd.audio import LogMelSpectrogram, LinearSpectrogram
    sr, n_fft, hop, pad, n_mels = (int(v) for v in gold[case + "/cfg"])
    lm = LogMelSpectrogram(sr, n_fft, n_fft, hop, 0.0, None, pad, n_mels, False, "reflect", "slaney").cuda()
    lin = LinearSpectrogram(n_fft, n_fft, hop, pad, False, "reflect").cuda()
    return lm, lin, (n_fft, hop, pad)


@pytest.mark.parametrize("case", CASES)
def test_case_matches_fixture_and_float64(gold, case):
    lm, lin, (n_fft, hop, pad) = _modules(gold, case)
    wave = gold[case + "/wave"]
    win, fb = lm.spectrogram.window.cpu().numpy(), lm.mel_scale.fb.cpu().numpy()
    mel = lm(torch.from_numpy(wave).cuda()).cpu().numpy()
    r64 = mr.log_mel(wave, win, fb, n_fft, hop, pad)
    ref = gold[case + "/mel"]
    torch_err = float(np.abs(ref - r64).max())
    err_fix, err_64 = float(np.abs(mel - ref).max()), float(np.abs(mel - r64).max())
    g64, gfix = (2 * torch_err, 3 * torch_err) if case == "tone" else (1e-3, 1e-3)
    # linear magnitude: the fixture's rows (item 0 only for the default case) through the (B, 1, L) input form
    nl = gold[case + "/linear"].shape[0]
    mag = lin(torch.from_numpy(wave[:nl]).cuda().unsqueeze(1)).cpu().numpy()
    l64 = mr.linear(wave[:nl], win, n_fft, hop, pad)
    lerr = float(np.abs(mag - l64).max() / np.abs(l64).max())
    lerr_fix = float(np.abs(mag - gold[case + "/linear"]).max() / np.abs(l64).max())
    ltorch = float(np.abs(gold[case + "/linear"] - l64).max() / np.abs(l64).max())
    print(f"{case}: log-mel native vs float64 {err_64:.2e}, vs fixture {err_fix:.2e}, torch fp32 vs float64 {torch_err:.2e} "
          f"(gates {g64:.1e} / {gfix:.1e});  linear rel native {lerr:.2e}, vs fixture {lerr_fix:.2e}, torch {ltorch:.2e}")
    assert mel.shape == ref.shape and mag.shape == gold[case + "/linear"].shape
    assert np.isfinite(mel).all() and err_64 <= g64 and err_fix <= gfix
    assert lerr <= 1e-5 and lerr_fix <= 1e-5
    if case == "silence":
        assert np.all(mag == np.float32(np.sqrt(np.float32(1e-6))))


def test_restatement_on_long_and_odd_shapes():
    """Beyond the fixture: 5 s at the default config (api.py's reference clip) and every scale on 2 s, against float64."""
    from stabletts_amd.audio import LogMelSpectrogram
    rng = np.random.Generator(np.random.PCG64(99))
    for n_mels, n_fft, secs in [(128, 2048, 5.0)] + [(m, n, 2.0) for m, n in zip([5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048])]:
        hop, pad = n_fft // 4, (n_fft - n_fft // 4) // 2
        L = int(secs * 44100) + 7
        wave = (0.3 * rng.standard_normal((2, L))).astype(np.float32)
        lm = LogMelSpectrogram(44100, n_fft, n_fft, hop, 0.0, None, pad, n_mels, False, "reflect", "slaney").cuda()
        mel = lm(torch.from_numpy(wave).cuda()).cpu().numpy()
        r64 = mr.log_mel(wave, lm.spectrogram.window.cpu().numpy(), lm.mel_scale.fb.cpu().numpy(), n_fft, hop, pad)
        err = float(np.abs(mel - r64).max())
        print(f"n_fft {n_fft}, {n_mels} mels, B=2 x {L}: log-mel vs float64 {err:.2e}")
        assert mel.shape == r64.shape and err <= 1e-3


def test_ragged_equals_each_utterance_alone_bitwise_and_repeats(gold):
    from stabletts_amd.audio import LogMelSpectrogram, LinearSpectrogram
    lm = LogMelSpectrogram(44100, 2048, 2048, 512, 0.0, None, 768, 128, False, "reflect", "slaney").cuda()
    lin = LinearSpectrogram(2048, 2048, 512, 768, False, "reflect").cuda()
    rng = np.random.Generator(np.random.PCG64(5))
    lengths = [769, 3072, 3209, 44100, 1000, 23456, 512 * 37]
    waves = [torch.from_numpy((0.2 * rng.standard_normal(n)).astype(np.float32)).cuda() for n in lengths]
    mels = lm.forward_ragged(waves)
    mags = lin.forward_ragged(waves)
    for w, m, g in zip(waves, mels, mags):
        assert torch.equal(m, lm(w[None])[0]) and torch.equal(g, lin(w[None])[0])
        assert m.shape == (128, lm.frames(w.numel())) and g.shape == (1025, lm.frames(w.numel()))
    again = lm.forward_ragged(waves)
    assert all(torch.equal(a, b) for a, b in zip(mels, again))
    # a padded batch: each row equals the row alone
    x = torch.stack([waves[3][:18000], waves[5][:18000], waves[6][:18000]])
    full = lm(x)
    assert all(torch.equal(full[b], lm(x[b:b + 1])[0]) for b in range(3))
    assert torch.equal(full, lm(x))


def test_loaded_window_and_filter_bank_are_honoured():
    from stabletts_amd.audio import LogMelSpectrogram
    lm = LogMelSpectrogram(44100, 1024, 1024, 256, 0.0, None, 384, 80, False, "reflect", "slaney").cuda()
    rng = np.random.Generator(np.random.PCG64(8))
    wave = torch.from_numpy((0.3 * rng.standard_normal((2, 9000))).astype(np.float32)).cuda()
    before = lm(wave)
    sd = lm.state_dict()
    win = torch.from_numpy(np.blackman(1024).astype(np.float32))
    fb = sd["mel_scale.fb"].cpu() * torch.from_numpy(rng.uniform(0.5, 1.5, size=tuple(sd["mel_scale.fb"].shape)).astype(np.float32))
    fb[:, 3] = 0.0                                              # an empty filter: log(1e-5)
    lm.load_state_dict({"spectrogram.window": win, "mel_scale.fb": fb})
    after = lm(wave).cpu().numpy()
    r64 = mr.log_mel(wave.cpu().numpy(), win.numpy(), fb.numpy(), 1024, 256, 384)
    err = float(np.abs(after - r64).max())
    print(f"blackman window + perturbed fb: log-mel vs float64 {err:.2e}")
    assert err <= 1e-3 and not np.allclose(after, before.cpu().numpy(), atol=1e-2)
    assert np.all(after[:, 3] == after[0, 3, 0]) and abs(float(after[0, 3, 0]) - np.log(1e-5)) <= 1e-5      # logf within 2 ulp
    with torch.no_grad():                                        # an in-place write bumps the version counter: re-read
        lm.spectrogram.window.fill_(1.0)
    r64 = mr.log_mel(wave.cpu().numpy(), np.ones(1024), fb.numpy(), 1024, 256, 384)
    assert float(np.abs(lm(wave).cpu().numpy() - r64).max()) <= 1e-3


def test_end_to_end_waveform_to_speaker_vector(gold):
    """api.py:72-73 -> models/model.py:79: fixture waveforms -> native LogMelSpectrogram -> native MelStyleEncoder, against the
    reference chain's c; gate of the style encoder's own test (max abs err / max|c| <= 1e-5)."""
    from stabletts_amd.audio import LogMelSpectrogram
    from stabletts_amd.reference_encoder import MelStyleEncoder
    lm = LogMelSpectrogram(44100, 2048, 2048, 512, 0.0, None, 768, 128, False, "reflect", "slaney").cuda()
    style = MelStyleEncoder(sw.N_MELS, style_vector_dim=sw.GIN, style_kernel_size=5, dropout=0.25)
    style.load_state_dict(sw.style_encoder_state_dict(), strict=True)
    style = style.cuda()
    c = style(lm(torch.from_numpy(gold["default/wave"]).cuda())).cpu().numpy()
    ref = gold["style_c"]
    err = float(np.abs(c - ref).max() / np.abs(ref).max())
    print(f"waveform -> mel -> c: max abs err / max|c| = {err:.2e}")
    assert c.shape == ref.shape and err <= 1e-5


def test_module_rules():
    from stabletts_amd.audio import LogMelSpectrogram
    lm = LogMelSpectrogram(44100, 2048, 2048, 512, 0.0, None, 768, 128, False, "reflect", "slaney").cuda()
    x = torch.zeros(1, 4096, device="cuda")
    with torch.enable_grad():
        with pytest.raises(NotImplementedError):
            lm(x.clone().requires_grad_(True))
        assert lm(x).shape == (1, 128, 8)                       # no input gradient asked: runs
    with pytest.raises(ValueError):
        lm(x.cpu())
    with pytest.raises(ValueError):
        lm(torch.zeros(1, 768, device="cuda"))                  # L <= pad: F.pad raises in the reference
    with pytest.raises(ValueError):
        lm(torch.zeros(2, 3, 4096, device="cuda"))
    assert lm(torch.zeros(1, 1, 769, device="cuda")).shape == (1, 128, 1)


def test_c_abi_ragged_and_handle_kinds():
    from stabletts_amd import _lib
    lib = _lib.load()
    mel = _lib.Engine(0, 0, 0, 0, 0, 0, 0, "f16", 0, mel=dict(n_fft=256, win_length=256, hop_length=64, pad=96, n_mels=40,
                                                              center=0, pad_mode=0))
    win = torch.hann_window(256).cuda()
    from stabletts_amd.audio import melscale_fbanks
    fb = melscale_fbanks(129, 0.0, 22050.0, 40, 44100, "slaney", "slaney").cuda()
    mel.load_state_dict({"spectrogram.window": win, "mel_scale.fb": fb})
    assert mel.mel_frames(97) == 1 + (97 + 192 - 256) // 64
    with pytest.raises(_lib.NativeError):
        mel.mel_frames(96)
    rng = np.random.Generator(np.random.PCG64(3))
    lens = [97, 1000, 333]
    wave = torch.from_numpy((0.5 * rng.standard_normal(sum(lens))).astype(np.float32)).cuda()
    so = [0, 97, 1097, 1430]
    T = [mel.mel_frames(n) for n in lens]
    fo = [0, T[0], T[0] + T[1], sum(T)]
    s = torch.cuda.current_stream().cuda_stream
    for output, rows in ((_lib.ST_MEL_LOG, 40), (_lib.ST_MEL_LINEAR, 129)):
        out = torch.full((rows * fo[-1],), float("nan"), device="cuda")
        mel.mel_forward_ragged(wave, so, fo, output, out, s)
        w = wave.cpu().numpy()
        for b in range(3):
            got = out[rows * fo[b]:rows * fo[b + 1]].view(rows, T[b]).cpu().numpy()
            seg = w[so[b]:so[b + 1]]
            r64 = (mr.log_mel(seg, win.cpu().numpy(), fb.cpu().numpy(), 256, 64, 96) if output == _lib.ST_MEL_LOG
                   else mr.linear(seg, win.cpu().numpy(), 256, 64, 96))[0]
            err = np.abs(got - r64).max() / (1.0 if output == _lib.ST_MEL_LOG else np.abs(r64).max())
            assert np.isfinite(got).all() and err <= 1e-3, (output, b, err)
    out = torch.empty(40 * fo[-1], device="cuda")
    so_p, fo_p = (ctypes.c_int64 * 4)(*so), (ctypes.c_int64 * 4)(*[0, T[0], T[0] + T[1], sum(T) + 1])
    assert lib.st_mel_forward_ragged(mel.handle, wave.data_ptr(), so_p, fo_p, 3, 0, out.data_ptr(), None) == _lib.ST_ERR_INVALID
    # handle kinds: the style encoder rejects a mel handle and the mel entry points reject a style-encoder handle
    sty = _lib.Engine(0, 0, 0, 0, 0, 0, 0, "f16", 0, style_encoder=dict(n_mel_channels=40, style_hidden=128, style_vector_dim=64,
                                                                         style_kernel_size=5, style_head=2))
    c = torch.empty(1, 64, device="cuda")
    m = torch.zeros(1, 40, 8, device="cuda")
    assert lib.st_style_encoder_forward(mel.handle, m.data_ptr(), None, c.data_ptr(), 1, 8, None) == _lib.ST_ERR_STATE
    assert lib.st_mel_forward(sty.handle, wave.data_ptr(), 1, 1000, out.data_ptr(), None) == _lib.ST_ERR_STATE
    so_p = (ctypes.c_int64 * 4)(*so)
    fo_p = (ctypes.c_int64 * 4)(*fo)
    assert lib.st_mel_forward_ragged(sty.handle, wave.data_ptr(), so_p, fo_p, 3, 0, out.data_ptr(), None) == _lib.ST_ERR_STATE
    assert lib.st_mel_frames(sty.handle, 1000) == _lib.ST_ERR_INVALID
    voc = torch.empty(1, 8 * 512, device="cuda")
    assert lib.st_vocos_forward(mel.handle, m.data_ptr(), voc.data_ptr(), 1, 8, None) == _lib.ST_ERR_STATE
    assert lib.st_repack(mel.handle, None) == _lib.ST_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    mel.close()
    sty.close()


def test_module_built_under_inference_mode():
    """Inference tensors carry no version counter: the handle keys on their address, and sync_weights() forces a re-read."""
    from stabletts_amd.audio import LogMelSpectrogram
    x = 0.2 * torch.randn(2, 9000, device="cuda")
    with torch.inference_mode():
        lm = LogMelSpectrogram(44100, 512, 512, 128, 0.0, None, 192, 80, False, "reflect", "slaney").cuda()
        a = lm(x)
        lm.mel_scale.fb.mul_(2.0)
        lm.sync_weights()
        b = lm(x)
    assert torch.allclose(b, torch.log(torch.clamp(2.0 * torch.exp(a), min=1e-5)), atol=1e-4)
