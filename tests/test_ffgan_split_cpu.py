"""Split-precision FireflyGAN vocoder ("f16_split" / "bf16_split") without a GPU: the hi + lo emulation, its accuracy on the default
configuration, the validation that keeps the new operand values away from every other engine kind, and the index map of the split
weight fragments (tests/ffgan_split_checks.py says what the emulation is)."""
import ctypes
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ffgan_restatement as R
from tests import ffgan_split_checks as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = ("f16_split", "bf16_split")


@pytest.fixture(scope="module")
def lib():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- emulation
def _bf16_by_hand(x32):
    """fp32 -> bf16 -> fp32 on the bits: round to nearest, ties to even."""
    b = x32.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def _round_by_hand(x32, dt):
    return x32.astype(np.float16).astype(np.float32) if dt == "f16_split" else _bf16_by_hand(x32)


def _probe_values():
    rng = np.random.default_rng(5)
    mags = np.exp2(rng.uniform(-30, 15.9, 4000))                    # 2^-30 ... 63 000: lo parts from zero through subnormal to normal
    tiny = np.exp2(rng.uniform(-24, -14, 500))                      # below f16's smallest normal: hi itself is subnormal
    edge = np.array([0.0, -0.0, 65504.0, 65503.5, 65519.0, -65519.0, 65488.0 + 15.99, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1.0, 1.0 + 2.0 ** -11,
                     1.0 + 2.0 ** -12, 1.0 + 3 * 2.0 ** -12, 0.1, 1 / 3])
    x = np.concatenate([mags * rng.choice([-1.0, 1.0], mags.size), tiny, edge])
    return x.astype(np.float32)


@pytest.mark.parametrize("dt", DTS)
def test_split_rounder_is_hi_plus_lo_by_hand(dt):
    x32 = _probe_values()
    hi = _round_by_hand(x32, dt)
    lo = _round_by_hand(x32 - hi, dt)                              # x - hi is exact in fp32
    want = hi.astype(np.float64) + lo.astype(np.float64)
    got = S.rounder(dt)(torch.from_numpy(x32.astype(np.float64))).numpy()
    assert got.dtype == np.float64 and np.array_equal(got, want)
    h, l = S.split_pair(torch.from_numpy(x32), S.SPLIT[dt])
    assert np.array_equal(h.numpy(), hi) and np.array_equal(l.numpy(), lo)
    # what the pair keeps: 2 x (mantissa bits) of the value, down to the format's smallest subnormal
    mant, quantum = (11, 2.0 ** -24) if dt == "f16_split" else (8, 2.0 ** -133)
    err = np.abs(want - x32.astype(np.float64))
    assert np.all(err <= np.maximum(np.abs(x32) * 2.0 ** (-2 * mant), quantum / 2))
    assert (x32 == 0).sum() == 2 and np.all(got[x32 == 0] == 0.0)
    # the plain names still round once, and float64 in is rounded to fp32 first
    assert np.array_equal(S.rounder("f16")(torch.from_numpy(x32.astype(np.float64))).numpy(), x32.astype(np.float16).astype(np.float64))
    y = torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64)
    assert float(S.rounder(dt)(y)) == 1.0
    assert S.rounder(None)(y) is y and R.rounder is S._plain_rounder      # the wrapper stands in only inside forward_emulated


def test_subnormal_lo_parts_survive_in_f16():
    """lo of a value around 1e-2 lies below 2^-14: torch's CPU f16 keeps it (the emulation's figures rest on that)."""
    x = torch.tensor([0.01234567], dtype=torch.float32)
    hi, lo = S.split_pair(x, torch.float16)
    assert 0 < abs(float(lo)) < 2.0 ** -14 and float(hi) + float(lo) != float(hi)
    assert abs(float(hi.double() + lo.double()) - float(x.double())) <= 2.0 ** -25


@pytest.mark.parametrize("dt", DTS)
def test_emulated_split_audio_is_within_1e_4_of_the_fixture(dt):
    """DEFAULT 1x24 against the real module's float64 fixture.  Measured: 2.7e-6 (f16_split), 1.8e-5 (bf16_split) -- against 1.58e-3 with
    f16 operands rounded once.  This pins the emulation, not the device."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ffgan_outputs.npz"))
    B, T = R.CASES[0]
    assert (B, T) == (1, 24)
    sd = R.make_state_dict(R.DEFAULT, R.SEED)
    out = S.forward_emulated(sd, R.DEFAULT, R.make_mel(B, T, 128, R.MEL_SEED), dt)
    e = {n: R.rel_max(out[n], gold[f"{B}x{T}/{n}"]) for n in ("audio", "encoder", "pre_tanh")}
    print(f"ffgan_split_emulation default {B}x{T} {dt}: " + "  ".join(f"{n} {v:.3e}" for n, v in e.items()))
    assert 0 < e["audio"] <= 1e-4, e
    assert e["audio"] < 0.05 * float(gold[f"{B}x{T}/emul_f16"][0][0])      # far below the single rounding it replaces


# ---------------------------------------------------------------- validation before the device
_DIT = dict(noise_channels=128, hidden_channels=256, filter_channels=1024, n_heads=4, n_layers=6, kernel_size=3, gin_channels=256)
OTHER_KINDS = {
    "decoder": {},
    "text_encoder": dict(text_encoder_vocab=401),
    "vocoder": dict(vocoder=dict(input_channels=128, dim=512, intermediate_dim=1536, num_layers=8, n_fft=2048, hop_length=512)),
    "style_encoder": dict(style_encoder=dict(n_mel_channels=100, style_hidden=128, style_vector_dim=256, style_kernel_size=5, style_head=2)),
    "duration_predictor": dict(duration_predictor=dict(in_channels=256, filter_channels=256, kernel_size=3, gin_channels=256)),
    "mel": dict(mel=dict(n_fft=1024, win_length=1024, hop_length=256, pad=384, n_mels=100, center=0, pad_mode=0)),
    "period_discriminator": dict(period_discriminator=dict(period=2, lrelu_slope=0.1)),
    "resolution_discriminator": dict(resolution_discriminator=dict(window_length=1024, lrelu_slope=0.1, **{f"band_lo{c}": c for c in range(5)},
                                                                   **{f"band_hi{c}": c + 1 for c in range(5)})),
}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", sorted(OTHER_KINDS))
def test_engine_rejects_split_names_for_every_other_kind(lib, kind, dt):
    """In Python, as a ValueError: the name is in OPERAND_DTYPES, and no st_create_* but st_create_ffgan may see its value."""
    from stabletts_amd import _lib
    assert dt in _lib.OPERAND_DTYPES and dt in _lib.SPLIT_OPERAND_DTYPES
    with pytest.raises(ValueError, match="FireflyGAN vocoder only"):
        _lib.Engine(*(_DIT[k] for k in _DIT), dt, 0, **OTHER_KINDS[kind])


@pytest.mark.parametrize("value", [2, 3])
def test_other_creators_answer_invalid_for_the_split_values(lib, value):
    from stabletts_amd import _lib
    assert (_lib.ST_OPERAND_BF16_SPLIT, _lib.ST_OPERAND_F16_SPLIT) == (2, 3)
    h = ctypes.c_void_p()
    dit = _lib.StConfig(**_DIT, operand_dtype=value)
    voc = _lib.StVocosConfig(**OTHER_KINDS["vocoder"]["vocoder"], operand_dtype=value)
    for rc in (lib.st_create(ctypes.byref(dit), 0, ctypes.byref(h)), lib.st_create_text_encoder(ctypes.byref(dit), 401, 0, ctypes.byref(h)),
               lib.st_create_vocoder(ctypes.byref(voc), 0, ctypes.byref(h))):
        assert rc == _lib.ST_ERR_INVALID and b"operand_dtype" in lib.st_last_error(None)      # before any device call
    assert not h.value


@pytest.mark.parametrize("dt", DTS)
def test_ffgan_creator_accepts_the_split_values(lib, dt):
    """Past the configuration checks the next failure is the device's; the same through _lib.Engine."""
    from stabletts_amd import _lib
    fields = _lib.ffgan_config_fields(R.small_config()["backbone"], R.small_config()["head"])
    cfg = _lib.StFfganConfig(**{**fields, "operand_dtype": _lib.OPERAND_DTYPES[dt]})
    h = ctypes.c_void_p()
    rc = lib.st_create_ffgan(ctypes.byref(cfg), 0, ctypes.byref(h))
    if torch.cuda.is_available():
        assert rc == 0, lib.st_last_error(None)
        lib.st_destroy(h)
        _lib.Engine(0, 0, 0, 0, 0, 0, 0, dt, 0, ffgan=fields).close()
    else:
        assert rc == _lib.ST_ERR_HIP and b"device" in lib.st_last_error(None)
        with pytest.raises(_lib.NativeError, match="device"):
            _lib.Engine(0, 0, 0, 0, 0, 0, 0, dt, 0, ffgan=fields)
    for bad in (4, -1):
        cfg.operand_dtype = bad
        assert lib.st_create_ffgan(ctypes.byref(cfg), 0, ctypes.byref(h)) == _lib.ST_ERR_INVALID


@pytest.mark.parametrize("dt", DTS)
def test_module_layout_pickle_and_wrapper_with_a_split_dtype(tmp_path, dt):
    from stabletts_amd.ffgan import FireflyGANBase, FireflyGANBaseWrapper
    sd = R.make_state_dict(R.DEFAULT, R.SEED)
    m = FireflyGANBase(operand_dtype=dt)
    assert m.operand_dtype == dt and FireflyGANBase().operand_dtype == "f16"
    assert list(m.state_dict()) == [n for n, _ in R.param_shapes(R.DEFAULT)] and len(m.state_dict()) == 471
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for mod in (m, FireflyGANBase()):       # pickling: as for the other dtypes -- torch serialises weight-normed modules through state_dict() only
        with pytest.raises(RuntimeError, match="state_dict"):
            pickle.dumps(mod)
    back = FireflyGANBase(operand_dtype=dt)
    back.load_state_dict(m.state_dict(), strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in back.state_dict().items())
    path = str(tmp_path / "generator.ckpt")
    torch.save(sd, path)
    w = FireflyGANBaseWrapper(path, operand_dtype=dt)
    assert w.model.operand_dtype == dt and not w.model.training
    assert FireflyGANBaseWrapper(path).model.operand_dtype == "f16"
    with pytest.raises(ValueError, match="no CPU fallback"):
        w(torch.zeros(1, 128, 4))


# ---------------------------------------------------------------- the split packing's index map
# planes: 1 = the default mode, 2 = f16 pairs (hi, lo), 3 = bf16 triples (hi, mid, lo); the split K chunk is 64 channels in both
def frag_map(cout, cin, taps, u, planes):
    """Restatement of ffgan_launch.h's ffg_frag_source / ffg_frag_offset: for every element idx of the hi stream
    [tile][chunk][k-step][lane][8] -> (index into v or -1, scale row or -1, [offset of the element's part p for p in range(planes)])."""
    kc = min(cin, 64 if planes > 1 else 128)
    nchunks, ksc = cin // kc, (taps * kc + 31) // 32
    n = (cout // 16) * nchunks * ksc * 512
    idx = np.arange(n, dtype=np.int64)
    e, lane, rest = idx & 7, (idx >> 3) & 63, idx >> 9
    ks, ch, tile = rest % ksc, (rest // ksc) % nchunks, rest // (ksc * nchunks)
    co, kk = tile * 16 + (lane & 15), ks * 32 + 8 * (lane >> 4) + e
    tap, ci = kk // kc, ch * kc + kk % kc
    if u == 0:
        src, row, ok = (co * cin + ci) * taps + tap, co, tap < taps
    else:
        Co = cout // u
        r, c = co // Co, co % Co
        j = r + u // 2 - u * (tap - 1)
        src, row, ok = (ci * Co + c) * (2 * u) + j, ci, (tap < taps) & (j >= 0) & (j < 2 * u)
    src, row = np.where(ok, src, -1), np.where(ok, row, -1)
    if planes > 1:
        return src, row, [(idx >> 9) * 512 * planes + p * 512 + (idx & 511) for p in range(planes)]
    return src, row, [idx]


def read_side(stream, cout, cin, taps, planes, plane):
    """What ffg_conv_kernel's k-loop multiplies a patch element (tap, ci) with: the dense W[co][tap][ci] recovered from the 16-bit
    buffer by the kernel's own addressing (shift / mask form), and the largest |weight| it meets in the K padding."""
    kc = min(cin, 64 if planes > 1 else 128)
    lg, nchunks, ksc = kc.bit_length() - 1, cin // kc, (taps * kc + 31) >> 5
    WL = 512 * planes                                              # 16-bit elements per k-step of one tile
    W = np.zeros((cout, taps, cin))
    pad = 0.0
    for tile in range(cout // 16):
        for ch in range(nchunks):
            for ks in range(ksc):
                base = ((tile * nchunks + ch) * ksc + ks) * WL + plane * 512
                for lane in range(64):
                    g, fl = lane >> 4, lane & 15
                    kk = ks * 32 + 8 * g
                    tap, ci = kk >> lg, kk & (kc - 1)
                    frag = stream[base + lane * 8: base + lane * 8 + 8]
                    if tap >= taps:
                        pad = max(pad, float(np.abs(frag).max()))
                    else:
                        W[tile * 16 + fl, tap, ch * kc + ci: ch * kc + ci + 8] = frag
    return W, pad


def _packed(v, scale, cout, cin, taps, u, planes):
    """Every part's stream in one buffer as the packing kernel writes them, in float64 without rounding (part p holds 0.5^p * value: it marks the plane)."""
    src, row, offs = frag_map(cout, cin, taps, u, planes)
    val = np.where(src >= 0, v.reshape(-1)[np.maximum(src, 0)] * scale[np.maximum(row, 0)], 0.0)
    buf = np.full(len(src) * planes, np.nan)
    for p, off in enumerate(offs):
        buf[off] = 0.5 ** p * val
    assert not np.isnan(buf).any()                                 # the offsets cover the buffer exactly once
    return buf


@pytest.mark.parametrize("planes", [3, 2, 1])
@pytest.mark.parametrize("cout,cin,taps", [(32, 128, 3), (16, 16, 3), (48, 256, 5), (16, 64, 13), (32, 32, 1)])
def test_fragment_map_of_a_plain_conv(cout, cin, taps, planes):
    """cin 128 and 256 are 2 and 4 chunks at the split kc = 64 (1 and 2 at 128); 16 x 3 and 32 x 1 pad K to a multiple of 32."""
    rng = np.random.default_rng(cout + cin + taps)
    v, scale = rng.standard_normal((cout, cin, taps)), rng.uniform(0.5, 2.0, cout)
    buf = _packed(v, scale, cout, cin, taps, 0, planes)
    want = (v * scale[:, None, None]).transpose(0, 2, 1)           # [co][tap][ci]
    for plane in range(planes):
        W, pad = read_side(buf, cout, cin, taps, planes, plane)
        assert pad == 0.0 and np.array_equal(W, want * 0.5 ** plane)


@pytest.mark.parametrize("planes", [3, 2, 1])
@pytest.mark.parametrize("cin,Co,u", [(128, 16, 4), (32, 16, 2), (256, 8, 6)])
def test_fragment_map_of_a_polyphase_transposed_conv(cin, Co, u, planes):
    """Against the restatement's polyphase_weight, and through it against F.conv_transpose1d."""
    rng = np.random.default_rng(cin + Co + u)
    wt, scale = rng.standard_normal((cin, Co, 2 * u)), rng.uniform(0.5, 2.0, cin)      # weight norm over dim 0 = the input channel
    cout = u * Co
    buf = _packed(wt, scale, cout, cin, 3, u, planes)
    folded = torch.from_numpy(wt * scale[:, None, None])
    want = R.polyphase_weight(folded, u).numpy().transpose(0, 2, 1)                     # (u * Co, 3, cin)
    for plane in range(planes):
        W, pad = read_side(buf, cout, cin, 3, planes, plane)
        assert pad == 0.0 and np.array_equal(W, want * 0.5 ** plane)
    x = torch.from_numpy(rng.standard_normal((1, cin, 7)))
    W, _ = read_side(buf, cout, cin, 3, planes, 0)
    y = F.conv1d(x, torch.from_numpy(W.transpose(0, 2, 1).copy()), None, padding=1).view(1, u, Co, 7).permute(0, 2, 3, 1).reshape(1, Co, 7 * u)
    assert float((y - F.conv_transpose1d(x, folded, None, stride=u, padding=u // 2)).abs().max()) <= 1e-12


def test_the_kernels_index_function_is_the_restated_map(tmp_path):
    """ffg_frag_source / ffg_frag_offset compiled for the host (no GPU, no sanitizer) against frag_map."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "ffgan_pack_index_check")
    src = os.path.join(ROOT, "tests", "host", "ffgan_pack_index_check.cpp")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for cout, cin, taps, u, planes in [(32, 128, 3, 0, 2), (16, 16, 3, 0, 2), (16, 64, 13, 0, 3), (64, 128, 3, 4, 2), (48, 256, 3, 6, 3), (32, 256, 5, 0, 1),
                                       (64, 128, 3, 4, 1), (32, 128, 3, 0, 3)]:
        out = str(tmp_path / "table.bin")
        r = subprocess.run([exe, str(cout), str(cin), str(taps), str(u), str(planes), out], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        table = np.fromfile(out, dtype=np.int64).reshape(-1, 5)
        src_want, row_want, offs = frag_map(cout, cin, taps, u, planes)
        assert len(table) == len(src_want)
        valid = src_want >= 0
        assert np.array_equal(table[:, 0], src_want) and np.array_equal(table[valid, 1], row_want[valid])
        for p in range(3):
            assert np.array_equal(table[:, 2 + p], offs[p] if p < planes else np.full(len(table), -1))
