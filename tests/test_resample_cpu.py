"""The sinc resampler without a GPU (stabletts_amd/audio.py: resample, resample_ragged, Resample, load_and_resample_wav): the compact
tap table against the dense kernel, the torch fallback against an independent float64 gather-sum, what the filter does to a tone and
to a constant, the argument errors, the C entry points' host-side checks, and the WAV reader."""
import ctypes
import math
import struct
import wave

import pytest
import torch

from tests import resample_restatement as R

CASES = list(zip(R.CONFIGS, R.IDS))
# the dense fallback at 8000 -> 44101 builds a (44101, 8014) float64 kernel (2.8 GB): its CPU checks run the other eight
FALLBACK_CASES = [c for c in CASES if c[1] != "8000-44101"]
HANN_CASES = CASES[:6]


def _param(cases):
    return pytest.mark.parametrize("cfg", [c[0] for c in cases], ids=[c[1] for c in cases])


@_param(CASES)
def test_compact_table_is_the_dense_kernels_kept_band(cfg, request):
    from stabletts_amd import audio
    o, n, kw = cfg
    orig, new, _, width, scale = R.geometry(o, n, **kw)
    tab = audio.resample_table(o, n, **kw)
    S, taps, first = tab["S"], tab["taps"], tab["first"].long()
    assert (tab["orig"], tab["new"], tab["width"]) == (orig, new, width)
    assert taps.shape == (S, new) and taps.dtype == torch.float32 and taps.is_contiguous()
    assert first.shape == (new,) and tab["first"].dtype == torch.int32
    assert new * S <= audio.RESAMPLE_MAX_TABLE
    hann = kw.get("resampling_method", "sinc_interp_hann") == "sinc_interp_hann"
    s = torch.arange(S)[None]
    longest, worst_dropped = 0, 0.0
    for lo in range(0, new, R.PHASE_BLOCK):
        hi = min(new, lo + R.PHASE_BLOCK)
        t = R.times(o, n, (lo, hi), **kw)
        k32 = R.kernel_at(t, scale, **kw).float()                     # = R.dense_kernel(o, n, (lo, hi), **kw)
        keep, k_first, count, contiguous = R.band(t, **kw)
        assert contiguous and int(count.min()) >= 1
        assert torch.equal(first[lo:hi], k_first - width)
        want = torch.where(s < count[:, None], k32.gather(1, (k_first[:, None] + s).clamp(max=k32.shape[1] - 1)), torch.zeros(()))
        assert torch.equal(taps[:, lo:hi].t().contiguous().view(torch.int32), want.view(torch.int32))      # bit for bit, padding +0
        if not bool(keep.all()):
            worst_dropped = max(worst_dropped, float(k32[~keep].abs().max()))
        longest = max(longest, int(count.max()))
    assert S == longest
    assert worst_dropped == 0.0 if hann else worst_dropped <= 2.0 ** -60 * scale
    if request.node.callspec.id in R.S_EXPECTED:
        assert S == R.S_EXPECTED[request.node.callspec.id]
    if request.node.callspec.id == "48000-44100":
        assert taps.numel() == 2058
    assert audio.resample_table(o, n, **kw)["taps"] is taps              # cached


def _lengths(o, n, kw):
    orig, _, _, width, _ = R.geometry(o, n, **kw)
    return [L for L in (1, width, orig - 1, orig, orig + 1, 2 * orig + 3) if L > 0]


@_param(FALLBACK_CASES)
def test_fallback_against_the_direct_sum(cfg):
    from stabletts_amd.audio import resample
    o, n, kw = cfg
    orig, new = R.geometry(o, n, **kw)[:2]
    g = torch.Generator().manual_seed(11)
    for L in _lengths(o, n, kw):
        x = torch.randn(L, generator=g, dtype=torch.float64)
        y64 = resample(x, o, n, **kw)
        want64 = R.direct(x, o, n, taps=torch.float64, **kw)
        assert y64.dtype == torch.float64 and y64.shape == (math.ceil(new * L / orig),) == want64.shape
        assert float((y64 - want64).abs().max()) <= 1e-12, L
        y32 = resample(x.float(), o, n, **kw)
        want32 = R.direct(x.float(), o, n, **kw)
        assert y32.dtype == torch.float32 and y32.shape == want32.shape
        assert float((y32.double() - want32).abs().max()) <= 64 * 2.0 ** -24 * float(want32.abs().max()), L


def test_fallback_shapes_equal_rates_and_gradients():
    from stabletts_amd.audio import Resample, resample, resample_ragged
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 3, 331, generator=g)
    y = resample(x, 48000, 44100)
    assert y.shape == (2, 3, math.ceil(147 * 331 / 160))
    for a in range(2):
        for b in range(3):
            assert torch.equal(y[a, b], resample(x[a, b], 48000, 44100))
            want = R.direct(x[a, b], 48000, 44100)
            assert float((y[a, b].double() - want).abs().max()) <= 64 * 2.0 ** -24 * float(want.abs().max())
    assert resample(x, 44100, 44100) is x and resample(x, 16000, 16000.0) is x
    assert resample(x[:, :, :0], 48000, 44100).shape == (2, 3, 0)
    # torchaudio's reduction by the greatest common divisor: 96000 -> 88200 is 48000 -> 44100
    assert torch.equal(resample(x, 96000, 88200), y)
    # the module and the ragged form are the function
    m = Resample(48000, 44100)
    assert torch.equal(m(x), y) and list(m.state_dict()) == [] and list(m.buffers()) == []
    waves = [x[0, 0], x[1, 2, :100], x[0, 1, :1]]
    out = resample_ragged(waves, 48000, 44100)
    assert isinstance(out, list) and all(torch.equal(a, resample(w, 48000, 44100)) for a, w in zip(out, waves))
    assert all(torch.equal(a, b) for a, b in zip(m.forward_ragged(waves), out))
    assert resample_ragged([], 48000, 44100) == [] and resample_ragged(waves, 8000, 8000)[1] is waves[1]
    k = Resample(44100, 16000, "sinc_interp_kaiser", 64, 0.9475937167399596, None)
    assert torch.equal(k(x), resample(x, 44100, 16000, 64, 0.9475937167399596, "sinc_interp_kaiser"))
    # gradients flow through the fallback: the filter is linear, so d sum(y w) / dx is the transposed filter applied to w
    xg = torch.randn(1, 200, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(1, math.ceil(147 * 200 / 160), generator=g, dtype=torch.float64)
    out = resample(xg, 48000, 44100)
    assert out.requires_grad
    (out * w).sum().backward()
    eye = torch.eye(200, dtype=torch.float64)
    jac = torch.stack([R.direct(eye[p], 48000, 44100, taps=torch.float64) for p in range(200)])          # (L, L_out)
    assert float((xg.grad[0] - jac @ w[0]).abs().max()) <= 1e-12
    h = torch.randn(1, 64, generator=g).half()
    assert resample(h, 22050, 44100).dtype == torch.float16
    with pytest.raises(TypeError, match="floating point"):
        resample(torch.zeros(1, 8, dtype=torch.int16), 22050, 44100)


@_param(HANN_CASES)
def test_a_tone_and_a_constant_come_out_as_themselves(cfg):
    """The width-6 Hann filter's passband ripple: a 1 kHz tone and a constant, away from the ends, within 1.5e-3 (measured:
    tone 1.1e-4 .. 7.3e-4, constant 4.6e-4 .. 8.8e-4 over these six conversions)."""
    o, n, kw = cfg
    L = 4000
    tone = torch.sin(2 * math.pi * 1000.0 * torch.arange(L, dtype=torch.float64) / o)
    y = R.dense(torch.stack([tone, torch.ones(L, dtype=torch.float64)]), o, n, taps=torch.float64, **kw)
    want = torch.sin(2 * math.pi * 1000.0 * torch.arange(y.shape[1], dtype=torch.float64) / n)
    mid = slice(200, y.shape[1] - 200)
    e_tone, e_const = float((y[0] - want)[mid].abs().max()), float((y[1] - 1)[mid].abs().max())
    print(f"{o} -> {n}: tone error {e_tone:.2e}, constant error {e_const:.2e}")
    assert e_tone <= 1.5e-3 and e_const <= 1.5e-3


def test_argument_errors():
    from stabletts_amd import audio
    x = torch.zeros(1, 64)
    for bad in (dict(orig_freq=0), dict(new_freq=0), dict(orig_freq=-8000), dict(new_freq=-1), dict(orig_freq=44100.5),
                dict(new_freq=22050.25), dict(lowpass_filter_width=0), dict(lowpass_filter_width=-3),
                dict(resampling_method="linear"), dict(resampling_method="kaiser_best")):
        kw = dict(orig_freq=48000, new_freq=44100)
        kw.update(bad)
        with pytest.raises(ValueError):
            audio.resample(x, **kw)
        with pytest.raises(ValueError):
            audio.resample_ragged([x[0]], **kw)
        with pytest.raises(ValueError):
            audio.Resample(**kw)
    with pytest.raises(ValueError):
        audio.resample_ragged([x], 48000, 44100)                        # 1-D waveforms only
    # the native table's limit: 330007 -> 330000 keeps up to S = 13 taps for each of 330000 phases
    with pytest.raises(NotImplementedError, match=r"2\^22"):
        audio.resample_table(330007, 330000)
    with pytest.raises(NotImplementedError, match=r"2\^22"):
        audio.resample_table(4000037, 4000000)                          # refused before anything that size is built
    from stabletts_amd import audio_train
    for name in ("resample", "resample_ragged", "Resample", "load_and_resample_wav"):
        assert getattr(audio_train, name) is getattr(audio, name)


def test_abi_symbols_and_host_side_argument_checks():
    import os
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stabletts_hip.h")).read()
    for name in ("st_resample", "st_resample_chunk", "st_resample_max_tensors"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and f"int {name}(" in hdr, name
    assert lib.st_abi_version() == 4
    C, M = lib.st_resample_chunk(), lib.st_resample_max_tensors()
    # an entry of the table: two pointers, two 64-bit lengths, the first block (padded to 8 bytes) = 40 bytes
    assert C >= 256 and C % 256 == 0 and M >= 2 and M * 40 <= 4096 - 256
    INV = _lib.ST_ERR_INVALID
    i64s = lambda *v: (ctypes.c_int64 * len(v))(*v)       # noqa: E731
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)      # noqa: E731
    err = lambda: lib.st_last_error(None).decode()        # noqa: E731
    # fake but well-formed device addresses: every call below must return before anything is launched
    a, b, taps, first = 0x1000, 0x2000, 0x3000, 0x4000
    ok = [ptrs(a), ptrs(b), i64s(160), i64s(147), 1, 160, 147, taps, first, 14, None]
    idx = dict(x=0, y=1, in_len=2, out_len=3, n=4, orig=5, new=6, taps=7, first=8, S=9)

    def call(**over):
        args = list(ok)
        for k, v in over.items():
            args[idx[k]] = v
        rc = lib.st_resample(*args)
        assert rc == _lib.ST_OK or err(), over              # every refusal says why
        return rc

    for name in ("x", "y", "in_len", "out_len", "taps", "first"):
        assert call(**{name: None}) == INV and err() == "null argument", name
    for name in ("x", "y"):
        assert call(**{name: ptrs(None)}) == INV and err() == "null tensor pointer", name
        for off in (1, 2, 3):
            assert call(**{name: ptrs(a + off)}) == INV and err() == "tensor pointers must be 4-byte aligned", name
    assert call(taps=taps + 2) == INV and call(first=first + 1) == INV
    assert call(n=-1) == INV
    for name in ("orig", "new", "S"):
        assert call(**{name: 0}) == INV and call(**{name: -2}) == INV, name
    assert call(in_len=i64s(-1)) == INV and call(out_len=i64s(-147)) == INV and "length" in err()
    for wrong in (146, 148, 0, 160):
        assert call(out_len=i64s(wrong)) == INV and err() == "out_len must be ceil(new_ * in_len / orig)", wrong
    assert call(in_len=i64s(161), out_len=i64s(147)) == INV           # ceil(147 * 161 / 160) = 148
    assert call(in_len=i64s(2 ** 62), out_len=i64s(147)) == INV       # the product is formed without overflow
    assert call(new=1 << 20, S=5, in_len=i64s(0), out_len=i64s(0)) == _lib.ST_ERR_UNSUPPORTED and "2^22" in err()
    # nothing to launch: an empty list, entries of length 0 (their pointers are not looked at)
    assert call(n=0) == _lib.ST_OK and call(n=0, x=None, y=None, in_len=None, out_len=None) == _lib.ST_OK
    assert call(in_len=i64s(0), out_len=i64s(0)) == _lib.ST_OK
    assert call(x=ptrs(None, None), y=ptrs(None, None), in_len=i64s(0, 0), out_len=i64s(0, 0), n=2) == _lib.ST_OK
    # a bad entry beyond the first launch group is found before the first group is launched
    n = M + 2
    assert lib.st_resample(ptrs(*([a] * n)), ptrs(*([b] * (n - 1) + [b + 2])), i64s(*([160] * n)), i64s(*([147] * n)), n, 160, 147,
                           taps, first, 14, None) == INV
    assert lib.st_resample(ptrs(*([a] * n)), ptrs(*([b] * n)), i64s(*([160] * n)), i64s(*([147] * (n - 1) + [148])), n, 160, 147,
                           taps, first, 14, None) == INV


def test_a_cpu_waveform_never_loads_the_library(monkeypatch):
    from stabletts_amd import _lib, audio

    def boom():
        raise AssertionError("the CPU path must not touch libstabletts_hip.so")
    monkeypatch.setattr(_lib, "load", boom)
    x = torch.randn(2, 500, generator=torch.Generator().manual_seed(3))
    assert audio.resample(x, 24000, 44100).shape == (2, math.ceil(147 * 500 / 80))
    assert len(audio.resample_ragged([x[0], x[1, :9]], 24000, 44100)) == 2


# ---------------------------------------------------------------- the WAV reader
def _write_wav(path, samples, channels, width, rate):
    """samples: (frames, channels) integers in the width's range (unsigned for 8-bit)"""
    raw = bytearray()
    for frame in samples:
        for v in frame:
            raw += bytes([v]) if width == 1 else int(v).to_bytes(width, "little", signed=True)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(bytes(raw))


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_wav_decoding_is_exact_and_keeps_the_first_channel(tmp_path, width, channels):
    from stabletts_amd.audio import load_and_resample_wav
    bits = 8 * width
    lo, hi = (0, 255) if width == 1 else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    g = torch.Generator().manual_seed(100 * width + channels)
    v = torch.randint(lo, hi + 1, (257, channels), generator=g, dtype=torch.int64)
    v[0, :], v[1, :], v[2, 0] = lo, hi, (128 if width == 1 else 0)
    path = tmp_path / f"pcm{bits}_{channels}.wav"
    _write_wav(path, v.tolist(), channels, width, 44100)
    y = load_and_resample_wav(str(path), 44100)
    first = v[:, 0].double()
    want = ((first - 128) / 128 if width == 1 else first / 2.0 ** (bits - 1)).float()
    assert y.dtype == torch.float32 and y.shape == (1, 257) and y.device.type == "cpu"
    assert torch.equal(y[0], want)                                      # the same rate: the samples untouched
    assert float(y.min()) == -1.0 and float(y[0, 2]) == 0.0
    if width < 4:                                                       # up to 24 bits an fp32 holds every sample exactly
        assert float(y.max()) < 1.0
        assert torch.equal(y[0].double(), (first - 128) / 128 if width == 1 else first / 2.0 ** (bits - 1))


def test_wav_resampling_and_failures(tmp_path, capsys):
    from stabletts_amd.audio import load_and_resample_wav, resample
    g = torch.Generator().manual_seed(5)
    v = torch.randint(-20000, 20000, (480, 2), generator=g, dtype=torch.int64)
    path = tmp_path / "stereo48k.wav"
    _write_wav(path, v.tolist(), 2, 2, 48000)
    y = load_and_resample_wav(str(path), 44100)
    assert y.shape == (1, 441) and torch.equal(y, resample((v[:, 0].float() / 32768)[None], 48000, 44100))
    capsys.readouterr()
    assert load_and_resample_wav(str(tmp_path / "missing.wav"), 44100) is None
    assert "missing.wav" in capsys.readouterr().out
    # IEEE-float WAVE (format tag 3) is not PCM: reported, None
    data = struct.pack("<4f", 0.0, 0.5, -0.5, 0.25)
    fmt = struct.pack("<HHIIHH", 3, 1, 48000, 48000 * 4, 4, 32)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    (tmp_path / "float.wav").write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    assert load_and_resample_wav(str(tmp_path / "float.wav"), 44100) is None
    assert capsys.readouterr().out.strip()
    (tmp_path / "noise.wav").write_bytes(bytes(range(64)))
    assert load_and_resample_wav(str(tmp_path / "noise.wav"), 44100) is None
    assert capsys.readouterr().out.strip()
    # load_and_resample_audio is as it was: without torchaudio it raises the ImportError that names it
    from stabletts_amd.audio import load_and_resample_audio
    try:
        import torchaudio  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="torchaudio"):
            load_and_resample_audio(str(path), 44100)
