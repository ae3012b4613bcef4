"""The native sinc resampler on the GPU (stabletts_amd/audio.py: resample, resample_ragged, load_and_resample_wav; st_resample)
against the float64 dense restatement of tests/resample_restatement.py.

Parity gate: e_native <= 4 max(e_torch, 2^-24 max|y|), both errors max-abs against float64; e_torch is the error of the module's own
fp32 dense fallback (F.pad + conv1d) on the same GPU, 4 the project's usual bar over torch fp32's own error and the floor one fp32
rounding of the output.  tools/resample_parity.py records the measured ratios in profiles/resample_parity.txt.

Where a conversion cannot produce an output length asked for (22050 -> 44100 gives even lengths only) the next longer one is taken."""
import ctypes
import math
import wave

import pytest
import torch

from tests import resample_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = list(zip(R.CONFIGS, R.IDS))


def _chunk():
    from stabletts_amd import _lib
    return _lib.load().st_resample_chunk()


def _rand(L, seed):
    return torch.randn(L, generator=torch.Generator().manual_seed(seed))


def _length_for(n_out, orig, new):
    """the shortest input whose output has at least n_out samples"""
    L = (n_out * orig) // new
    while R.out_len(L, orig, new) < n_out:
        L += 1
    while L > 1 and R.out_len(L - 1, orig, new) >= n_out:
        L -= 1
    return L


def edge_lengths(o, n, kw, chunk):
    orig, new, _, width, _ = R.geometry(o, n, **kw)
    Ls = [1, width, orig - 1, orig + 1] + [_length_for(t, orig, new) for t in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1)]
    return sorted({L for L in Ls if L > 0})


def parity_inputs(o, n, kw, chunk):
    """The waveforms of one configuration's parity case (CPU fp32): every edge length, B = 3 rows, a (2, 3, L) batch."""
    orig, new = R.geometry(o, n, **kw)[:2]
    xs = [_rand(L, 1000 + L) for L in edge_lengths(o, n, kw, chunk)]
    L3 = _length_for(chunk + 1, orig, new)
    xs.append(_rand(3 * L3, 7).view(3, L3))
    xs.append(_rand(6 * (L3 + 5), 8).view(2, 3, L3 + 5))
    return xs


def fallback(x, o, n, kw):
    """The module's dense torch formulation on x's device: what a grad-enabled call runs."""
    from stabletts_amd.audio import resample
    with torch.enable_grad():
        y = resample(x.detach().clone().requires_grad_(True), o, n, **kw)
    assert y.requires_grad
    return y.detach()


def parity_errors(o, n, kw, chunk):
    """-> [(shape, e_native, e_torch, floor)] of one configuration, all against one evaluation of the float64 dense kernel"""
    from stabletts_amd.audio import resample
    orig, new = R.geometry(o, n, **kw)[:2]
    xs = parity_inputs(o, n, kw, chunk)
    truth = R.dense(xs, o, n, **kw)
    rows = []
    for x, want in zip(xs, truth):
        xg = x.to(DEV)
        y = resample(xg, o, n, **kw)
        assert y.dtype == torch.float32 and y.device == xg.device and not y.requires_grad
        assert y.shape == x.shape[:-1] + (math.ceil(new * x.shape[-1] / orig),) == want.shape
        yt = fallback(xg, o, n, kw)
        assert yt.shape == y.shape
        e_native = float((y.double().cpu() - want).abs().max())
        e_torch = float((yt.double().cpu() - want).abs().max())
        rows.append((tuple(x.shape), e_native, e_torch, 2.0 ** -24 * float(want.abs().max())))
    return rows


@pytest.mark.parametrize("cfg", [c[0] for c in CASES], ids=[c[1] for c in CASES])
def test_parity_against_the_float64_dense_restatement(cfg):
    o, n, kw = cfg
    rows = parity_errors(o, n, kw, _chunk())
    for shape, e_native, e_torch, floor in rows:
        print(f"{o} -> {n} {shape}: native {e_native:.3e}, torch fp32 {e_torch:.3e}, floor {floor:.3e}, ratio {e_native / max(e_torch, floor):.2f}")
    for shape, e_native, e_torch, floor in rows:
        assert e_native <= 4 * max(e_torch, floor), (shape, e_native, e_torch, floor)


# ---------------------------------------------------------------- bitwise properties
BITWISE = [(48000, 44100, {}), (22050, 44100, {}), (44100, 16000, R.KAISER)]


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def pool():
    """Per bitwise configuration: distinct waveforms (lengths 1, 2, a few short ones, one of several chunks) and each one's
    result alone."""
    from stabletts_amd.audio import resample
    out = {}
    with torch.no_grad():
        for k, (o, n, kw) in enumerate(BITWISE):
            orig, new = R.geometry(o, n, **kw)[:2]
            Ls = [1, 2, 5, orig + 1, _length_for(_chunk(), orig, new), _length_for(3 * _chunk() + 7, orig, new), 777]
            xs = [_rand(L, 50 * k + i).to(DEV) for i, L in enumerate(Ls)]
            out[k] = (xs, [resample(x, o, n, **kw) for x in xs])
    return out


@pytest.mark.parametrize("k", range(len(BITWISE)))
def test_ragged_is_each_waveform_alone_at_any_position_and_next_to_nan(pool, k):
    from stabletts_amd.audio import resample, resample_ragged
    o, n, kw = BITWISE[k]
    xs, alone = pool[k]
    got = resample_ragged(xs, o, n, **kw)
    assert len(got) == len(xs) and all(_same_bits(a, b) for a, b in zip(got, alone))
    assert all(_same_bits(a, b) for a, b in zip(resample_ragged(xs, o, n, **kw), alone))           # two runs agree
    assert all(_same_bits(resample(x, o, n, **kw), a) for x, a in zip(xs, alone))
    order = [3, 6, 0, 5, 2, 1, 4]
    got = resample_ragged([xs[i] for i in order], o, n, **kw)
    assert all(_same_bits(got[p], alone[i]) for p, i in enumerate(order))
    for keep in (0, 3, 5):                                                                    # every neighbour NaN
        nan = [x if i == keep else torch.full_like(x, float("nan")) for i, x in enumerate(xs)]
        got = resample_ragged(nan, o, n, **kw)
        assert _same_bits(got[keep], alone[keep])
        assert all(bool(torch.isnan(g).all()) for i, g in enumerate(got) if i != keep)
    # as rows of a batch
    rows = torch.stack([xs[6], xs[6].flip(0), torch.full_like(xs[6], float("nan"))])
    y = resample(rows, o, n, **kw)
    assert _same_bits(y[0], alone[6]) and _same_bits(y[1], resample(xs[6].flip(0), o, n, **kw))


@pytest.mark.parametrize("k", range(len(BITWISE)))
def test_results_do_not_change_with_the_address(pool, k):
    """Inputs at 0 .. 3 floats past a 16-byte boundary inside a flat buffer, outputs likewise (a leading waveform of 1 .. 4
    output samples shifts every later result inside resample_ragged's one output buffer)."""
    from stabletts_amd.audio import resample_ragged
    o, n, kw = BITWISE[k]
    orig, new = R.geometry(o, n, **kw)[:2]
    xs, alone = pool[k]
    seen = set()
    for off_in in range(4):
        flat = torch.full((sum(x.numel() for x in xs) + 8 * len(xs),), float("nan"), device=DEV)
        assert flat.data_ptr() % 16 == 0
        views, at = [], 0
        for x in xs:
            at = (at + 3) // 4 * 4 + off_in
            views.append(flat[at:at + x.numel()].copy_(x))
            at += x.numel()
        assert all(v.data_ptr() % 16 == 4 * off_in for v in views)
        for lead in range(4):
            first = xs[6][:_length_for(lead + 1, orig, new)]                    # 1 .. 4 output samples in front
            got = resample_ragged([first] + views + [views[4]], o, n, **kw)
            seen |= {g.data_ptr() % 16 for g in got[1:]}
            assert all(_same_bits(g, a) for g, a in zip(got[1:], alone + [alone[4]])), (off_in, lead)
    assert seen == ({0, 8} if new == 2 else {0, 4, 8, 12})              # 22050 -> 44100: every output length is even


@pytest.mark.parametrize("count", ["M-1", "M", "M+1", "2M+2"])
def test_lists_across_the_launch_boundary(pool, count):
    from stabletts_amd import _lib
    from stabletts_amd.audio import resample_ragged
    M = _lib.load().st_resample_max_tensors()
    count = {"M-1": M - 1, "M": M, "M+1": M + 1, "2M+2": 2 * M + 2}[count]
    o, n, kw = BITWISE[0]
    xs, alone = pool[0]
    empty = torch.empty(0, device=DEV)
    # lengths 1 and 2 at the launch boundaries, an empty waveform in the middle (it takes no place in a launch)
    pick = [(3 * i + i // 7) % len(xs) for i in range(count)]
    for b in (0, M - 1, M, count - 1):
        if b < count:
            pick[b] = 0 if b % 2 == 0 else 1
    waves = [xs[i] for i in pick]
    waves.insert(count // 2, empty)
    got = resample_ragged(waves, o, n, **kw)
    assert got[count // 2].numel() == 0
    del got[count // 2]
    assert len(got) == count and all(_same_bits(g, alone[i]) for g, i in zip(got, pick))


def test_guards_around_every_input_and_output_stay_nan(pool):
    """st_resample on views carved out of flat buffers with NaN guard elements on both sides of every waveform: a read outside
    [0, L_in) would make an output NaN, a write outside [0, L_out) would overwrite a guard."""
    from stabletts_amd import _lib
    from stabletts_amd.audio import resample_table
    lib = _lib.load()
    for k, (o, n, kw) in enumerate(BITWISE):
        xs, alone = pool[k]
        tab = resample_table(o, n, device=DEV, **kw)
        G = 5
        flat_in = torch.full((sum(x.numel() + G for x in xs) + G,), float("nan"), device=DEV)
        flat_out = torch.full((sum(a.numel() + G for a in alone) + G,), float("nan"), device=DEV)
        ins, outs, a_in, a_out = [], [], G, G
        for x, a in zip(xs, alone):
            ins.append(flat_in[a_in:a_in + x.numel()].copy_(x))
            outs.append(flat_out[a_out:a_out + a.numel()])
            a_in, a_out = a_in + x.numel() + G, a_out + a.numel() + G
        m = len(xs)
        rc = lib.st_resample((ctypes.c_void_p * m)(*[t.data_ptr() for t in ins]), (ctypes.c_void_p * m)(*[t.data_ptr() for t in outs]),
                             (ctypes.c_int64 * m)(*[t.numel() for t in ins]), (ctypes.c_int64 * m)(*[t.numel() for t in outs]), m,
                             tab["orig"], tab["new"], tab["taps"].data_ptr(), tab["first"].data_ptr(), tab["S"],
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == _lib.ST_OK, lib.st_last_error(None).decode()
        torch.cuda.synchronize()
        written = torch.zeros_like(flat_out, dtype=torch.bool)
        a_out = G
        for a in alone:
            written[a_out:a_out + a.numel()] = True
            a_out += a.numel() + G
        assert bool(torch.isnan(flat_out[~written]).all()) and int((~written).sum()) == G * (m + 1)
        assert not bool(torch.isnan(flat_out[written]).any())
        assert all(_same_bits(g, a) for g, a in zip(outs, alone))


# ---------------------------------------------------------------- dispatch
def test_other_dtypes_keep_their_dtype_through_the_fallback():
    from stabletts_amd.audio import resample
    x = _rand(500, 21)
    want = R.dense(x, 48000, 44100)
    y64 = resample(x.double().to(DEV), 48000, 44100)
    assert y64.dtype == torch.float64 and y64.is_cuda
    assert float((y64.cpu() - R.dense(x, 48000, 44100, taps=torch.float64)).abs().max()) <= 1e-12
    y16 = resample(x.half().to(DEV), 48000, 44100)
    assert y16.dtype == torch.float16 and y16.is_cuda and y16.shape == want.shape
    assert float((y16.double().cpu() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())     # fp16 taps, samples and result


@pytest.mark.grad
def test_a_grad_enabled_waveform_takes_the_fallback(monkeypatch):
    from stabletts_amd import _lib, audio
    x = _rand(700, 22).to(DEV)
    native = audio.resample(x, 48000, 44100)                            # no grad needed: native
    key = audio._resample_key(48000, 44100, 6, 0.99, "sinc_interp_hann", None)
    dense = audio._resample_dense(x, key)

    def boom():
        raise AssertionError("a grad-enabled call must not reach the native path")
    monkeypatch.setattr(_lib, "load", boom)
    xg = x.clone().requires_grad_(True)
    y = audio.resample(xg, 48000, 44100)
    assert y.requires_grad and torch.equal(y.detach(), dense)
    y.square().sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    assert float((native - dense).abs().max()) <= 1e-5 * float(dense.abs().max())
    got = audio.resample_ragged([xg, xg[:10]], 48000, 44100)
    assert got[0].requires_grad and torch.equal(got[0].detach(), dense)
    with torch.no_grad():                                               # requires grad, autograd off: native again
        monkeypatch.undo()
        assert _same_bits(audio.resample(xg, 48000, 44100), native)


def test_a_cpu_waveform_never_touches_the_library(monkeypatch):
    from stabletts_amd import _lib, audio
    x = _rand(300, 23)

    def boom():
        raise AssertionError("the CPU path must not touch libstabletts_hip.so")
    monkeypatch.setattr(_lib, "load", boom)
    y = audio.resample(x, 48000, 44100)
    assert y.device.type == "cpu" and float((y.double() - R.dense(x, 48000, 44100)).abs().max()) <= 64 * 2.0 ** -24 * float(y.abs().max())


def test_file_to_log_mel(tmp_path):
    from stabletts_amd.audio import LogMelSpectrogram, load_and_resample_wav, resample
    v = (_rand(24000, 24) * 6000).round().clamp(-32768, 32767).to(torch.int16)
    left_right = torch.stack([v, v.flip(0)], 1).contiguous()
    path = str(tmp_path / "ref48k.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(48000)
        f.writeframes(left_right.numpy().tobytes())
    y = load_and_resample_wav(path, 44100, device=DEV)
    assert y.is_cuda and y.dtype == torch.float32 and y.shape == (1, 22050)
    samples = (v.float() / 32768)[None].to(DEV)
    want = resample(samples, 48000, 44100)
    assert _same_bits(y, want)
    mel = LogMelSpectrogram(44100, 2048, 2048, 512, 0.0, None, 768, 128, False, "reflect", "slaney").to(DEV)
    out = mel(y)
    assert out.shape == (1, 128, mel.frames(22050)) and bool(torch.isfinite(out).all())
    assert _same_bits(out, mel(want))
    same = load_and_resample_wav(path, 48000, device=DEV)              # the file's own rate: its samples, on the device
    assert same.is_cuda and _same_bits(same, samples)
