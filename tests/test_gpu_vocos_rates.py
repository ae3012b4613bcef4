"""The native Vocos vocoder at n_fft 1024 / 512 / 256 (hop_length n_fft / 4) and at mel widths that are no multiple of 64, against
the float64 oracle (oracle/vocos_oracle.py, pinned to the real module at such configurations by tests/test_vocos_rates_cpu.py).

What is new at these configurations (engine_vocos.cpp, vocos_kernels.hip) and which test reaches it:

    head planes of pitch round_up(n_fft / 2 + 1, 128): cout 1280 / 768 / 512   every test; the GEMM's tile switch points in
                                                                               test_head_tile_paths_vs_oracle
    inverse FFT with S = 2048 / n_fft frames per block                         R = 1, 6, 27, 260 rows: the last block is part-filled
    overlap-add with hop 256 / 128 / 64                                        T = 1 (one frame) .. 130; ragged: Tmax * hop % 256 != 0
    im2col rows of pitch round_up(7 M, 64) with a zero tail                    M = 80, 96, 16, 176, also on the n_fft 2048 ISTFT

Backbones have 1-2 layers and intermediate_dim 256, so each case takes well under a second.  Gates: TOL_AUDIO of
tests/test_gpu_vocos_shapes.py (1e-3 with f16 operands, 1e-2 with bf16, relative to max |ref| of the utterance); the ISTFT alone 2e-5
(tests/test_gpu_vocos.py::test_istft_head_alone_is_fp32_exact).  Every test prints its measured errors beside the gate.

Measured on one MI355X (profiles/vocos_rates_parity.txt): every case passes.  f16 waveform errors 5.9e-4 .. 9.95e-4; the shallow
backbones sit closer to the 1e-3 bar than the 8-layer preset does (5.5e-4 .. 8.5e-4 at the new n_fft against the preset's 6.3e-4): nearest
n_fft 512 / M 96 at 2 x 130 frames 9.95e-4 and n_fft 256 / M 176 at 3 x 9 frames 9.80e-4; the n_fft 2048 handle with the same backbone 6.7e-4 ..
7.7e-4 at M = 16 .. 176.  bf16 5.5e-3 .. 7.2e-3 (bar 1e-2).  The ISTFT alone 1.5e-7 .. 2.1e-7 (bar 2e-5).
"""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import vocos_oracle as vo
from oracle.make_golden_vocos import SD_SEED
from tests.test_gpu_vocos_shapes import TOL_AUDIO, _mel, _oracle, _rel, _state_dict, _vocoder, tile_of

pytestmark = pytest.mark.gpu

ISTFT_BAR = 2e-5
RATES = [(1024, 80), (512, 96), (256, 16), (256, 176)]        # (n_fft, M)
SHAPES = [(1, 1), (2, 3), (3, 9), (2, 130)]                   # R = 1, 6, 27, 260


def _fields(n_fft, M, dim=512, layers=2):
    return dict(n_fft=n_fft, hop_length=n_fft // 4, input_channels=M, dim=dim, intermediate_dim=256, num_layers=layers)


def _key(fields):
    return tuple(sorted(fields.items()))


@functools.lru_cache(maxsize=None)
def _voc(key, dtype):
    return _vocoder(dict(key), dtype)


def _check_dense(fields, dtype, B, T, seed, items=None):
    key = _key(fields)
    voc = _voc(key, dtype)
    hop = fields["hop_length"]
    audio = voc(torch.from_numpy(_mel(B, T, seed, fields["input_channels"])).cuda())
    assert audio.shape == (B, T * hop) and bool(torch.isfinite(audio).all())
    bad = []
    for i in (range(B) if items is None else items):
        ea = _rel(audio[i].cpu().numpy(), _oracle(key, B, T, seed, i)[1])
        print(f"{dtype} n_fft {fields['n_fft']} M {fields['input_channels']} dim {fields['dim']} B={B} T={T} item {i}: "
              f"audio {ea:.2e} (gate {TOL_AUDIO[dtype]:.0e})")
        if not ea < TOL_AUDIO[dtype]:
            bad.append((i, ea))
    assert not bad, bad


@pytest.mark.parametrize("B,T", SHAPES, ids=[f"B{B}T{T}" for B, T in SHAPES])
@pytest.mark.parametrize("n_fft,M", RATES, ids=[f"n{n}m{m}" for n, m in RATES])
def test_dense_vs_oracle(n_fft, M, B, T):
    """R = 1, 6, 27 and 260 rows: none a multiple of 8 and three no multiple of 2 or 4, so the part-filled last block of the inverse
    FFT runs at every n_fft; T = 1 is an utterance of one frame, T = 130 crosses the 64-frame im2col tile and the 128-row GEMM tile."""
    _check_dense(_fields(n_fft, M), "f16", B, T, 400 + T)


@pytest.mark.parametrize("n_fft,M", RATES[:3], ids=[f"n{n}m{m}" for n, m in RATES[:3]])
def test_dense_bf16_vs_oracle(n_fft, M):
    _check_dense(_fields(n_fft, M), "bf16", 2, 130, 530)


@pytest.mark.parametrize("dim", [768, 1024])
def test_dense_wider_backbones_vs_oracle(dim):
    _check_dense(_fields(1024, 80, dim=dim), "f16", 3, 9, 409)


@pytest.mark.parametrize("M", [16, 80, 96, 176])
def test_mel_widths_on_the_2048_istft(M):
    """n_fft 2048 / hop 512, whose ISTFT kernels are untouched: isolates the im2col rows of pitch round_up(7 M, 64)."""
    _check_dense(_fields(2048, M), "f16", 2, 130, 600 + M)


@pytest.mark.parametrize("n_fft,M", RATES[:3], ids=[f"n{n}m{m}" for n, m in RATES[:3]])
def test_istft_alone_is_fp32_exact(n_fft, M):
    """The ISTFT kernels are fp32: audio against the float64 istft_same of the captured head output.  R = 21 rows is no multiple of
    S = 2, 4 or 8, and with T = 7 interior samples sum four frames and edge samples fewer."""
    fields, (B, T, seed) = _fields(n_fft, M), (3, 7, 11)
    voc = _voc(_key(fields), "f16")
    bins, plane = n_fft // 2 + 1, (n_fft // 2 + 1 + 127) // 128 * 128
    eng = voc.engine()
    eng.debug_capture(True)
    try:
        audio = voc(torch.from_numpy(_mel(B, T, seed, M)).cuda()).cpu().numpy()
        ho = eng.debug_fetch("voc.head_out")
    finally:
        eng.debug_capture(False)
    assert ho.size == B * T * 2 * plane
    ho = ho.reshape(B, T, 2, plane)[..., :bins].astype(np.float64)
    mag = np.minimum(np.exp(ho[:, :, 0]), 1e2)
    S = (mag * (np.cos(ho[:, :, 1]) + 1j * np.sin(ho[:, :, 1]))).transpose(0, 2, 1)
    window = _state_dict(_key(fields))["head.istft.window"].astype(np.float64)
    err = _rel(audio, vo.istft_same(S, window, n_fft, n_fft // 4))
    print(f"n_fft {n_fft}: ISTFT alone {err:.2e} (gate {ISTFT_BAR:.0e})")
    assert err < ISTFT_BAR


# (n_fft, M, B, T): the head GEMM (EPI_F32, cout 1280 / 768 / 512) just below and just above each switch point of its tile
# (tests/test_vocos_rates_cpu.py::test_head_tile_switch_points); 3 x 3243 = 9729 rows also run the depthwise conv's
# four-frames-per-wave path (R >= 8192) with T % 4 == 3
TILE_BATCHES = [(1024, 80, 32, 100, "T64"), (1024, 80, 3, 1067, "T128"), (1024, 80, 76, 128, "T128"), (1024, 80, 3, 3243, "BIG"),
                (512, 96, 42, 128, "T64"), (512, 96, 19, 283, "T128"), (256, 16, 64, 128, "T64"), (256, 16, 3, 2731, "T128")]


@pytest.mark.parametrize("n_fft,M,B,T,tile", TILE_BATCHES, ids=[f"n{n}R{B * T}" for n, _, B, T, _ in TILE_BATCHES])
def test_head_tile_paths_vs_oracle(n_fft, M, B, T, tile):
    cout = 2 * ((n_fft // 2 + 1 + 127) // 128 * 128)
    assert tile_of(B * T, cout, "F32") == tile
    _check_dense(_fields(n_fft, M, layers=1), "f16", B, T, 700 + B, items=(0, B - 1))


def test_stale_workspace_does_not_reach_a_clean_call():
    """The im2col rows' zero tail (M = 80: columns 560 .. 575) is written on every call.  Calls whose mel is all NaN -- one at a smaller
    shape, whose NaN activations lie where the larger call's im2col rows come to lie, and one at the clean call's shape -- leave NaN
    all over the reused workspace; the clean call after them is finite and bitwise the same call on a fresh handle."""
    fields, (B, T, seed) = _fields(1024, 80), (2, 70, 21)
    mel = torch.from_numpy(_mel(B, T, seed, 80)).cuda()
    voc = _vocoder(fields, "f16")
    voc(mel)                                                            # sizes the workspace
    assert bool(torch.isnan(voc(torch.full((1, 80, 3), float("nan"), device="cuda"))).all())
    assert bool(torch.isnan(voc(torch.full_like(mel, float("nan")))).all())
    clean = voc(mel)
    fresh = _vocoder(fields, "f16")(mel)
    print(f"clean call after NaN calls: finite {bool(torch.isfinite(clean).all())}, bitwise the fresh handle's {torch.equal(clean, fresh)}")
    assert bool(torch.isfinite(clean).all()) and torch.equal(clean, fresh)


RAGGED = [(1024, 80, (9, 1, 5)), (1024, 80, (130, 70, 64, 65)), (256, 16, (9, 1, 5)), (256, 16, (130, 70, 64, 65)), (256, 16, (3, 7, 7, 2))]


@pytest.mark.parametrize("n_fft,M,lengths", RAGGED, ids=[f"n{n}-" + "_".join(map(str, ls)) for n, _, ls in RAGGED])
def test_ragged_is_bitwise_each_utterance_alone(n_fft, M, lengths):
    """forward_ragged with NaN in the mel beyond each length: every utterance is bitwise the dense call on it alone and zero from
    lengths[b] * hop on.  With hop 64 and Tmax = 9 or 7, Tmax * hop is no multiple of the overlap-add's 256-sample blocks: the
    sample after utterance b's last is utterance b + 1's first, and must be that utterance's own."""
    fields = _fields(n_fft, M)
    voc, hop, B, Tmax = _voc(_key(fields), "f16"), n_fft // 4, len(lengths), max(lengths)
    mel = torch.from_numpy(_mel(B, Tmax, 800 + Tmax, M)).cuda()
    for b, n in enumerate(lengths):
        mel[b, :, n:] = float("nan")
    audio = voc.forward_ragged(mel, list(lengths))
    assert audio.shape == (B, Tmax * hop)
    for b, n in enumerate(lengths):
        solo = voc(mel[b:b + 1, :, :n].contiguous())[0]
        same, tail = torch.equal(audio[b, :n * hop], solo), bool((audio[b, n * hop:] == 0).all())
        print(f"n_fft {n_fft} lengths {lengths} item {b}: bitwise the utterance alone {same}, zero tail {tail}")
        assert same and tail, b
        if b + 1 < B and (Tmax * hop) % 256:
            nxt = voc(mel[b + 1:b + 2, :, :lengths[b + 1]].contiguous())[0]
            assert audio.reshape(-1)[(b + 1) * Tmax * hop] == nxt[0]


@pytest.mark.parametrize("n_fft,M", [(1024, 80), (256, 16)])
def test_ragged_equal_lengths_is_bitwise_dense(n_fft, M):
    fields = _fields(n_fft, M)
    voc = _voc(_key(fields), "f16")
    mel = torch.from_numpy(_mel(3, 9, 809, M)).cuda()
    assert torch.equal(voc.forward_ragged(mel, [9, 9, 9]), voc(mel))


@pytest.mark.grad
def test_training_entries_refuse_and_no_grad_is_the_inference_path():
    """vocos_train.Vocos at (1024, 256, 80) constructs and loads; under autograd the native training forward refuses with
    ST_ERR_UNSUPPORTED (training keeps n_fft 2048 / hop 512 and mel widths in steps of 64); under no_grad it is the inference path."""
    from stabletts_amd import vocos_train
    from stabletts_amd._lib import NativeError, ST_ERR_UNSUPPORTED
    fields = _fields(1024, 80)
    m = vocos_train.Vocos(types.SimpleNamespace(**{k: fields[k] for k in ("input_channels", "dim", "intermediate_dim", "num_layers")}),
                          types.SimpleNamespace(n_fft=1024, hop_length=256))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _state_dict(_key(fields)).items()}, strict=True)
    m = m.to("cuda:0").train()
    mel = torch.from_numpy(_mel(2, 9, 31, 80)).cuda()
    with pytest.raises(NativeError) as ei:
        m(mel)
    assert ei.value.code == ST_ERR_UNSUPPORTED and "2048" in str(ei.value)
    with torch.no_grad():
        audio = m(mel)
    assert torch.equal(audio, _voc(_key(fields), "f16")(mel))


def test_front_end_to_vocoder_at_22050():
    """A waveform through the native LogMelSpectrogram of MelConfig(22050, 1024, 1024, 256, n_mels=80) and the native Vocos of the
    same config: frames(L) * 256 finite samples."""
    from stabletts_amd.audio import LogMelSpectrogram
    from stabletts_amd.vocos import Vocos
    L = 11025
    lm = LogMelSpectrogram(22050, 1024, 1024, 256, 0.0, None, (1024 - 256) // 2, 80, False, "reflect", "slaney").to("cuda:0")
    voc = Vocos(types.SimpleNamespace(input_channels=80, dim=512, intermediate_dim=1536, num_layers=8),
                types.SimpleNamespace(n_fft=1024, hop_length=256)).to("cuda:0")
    g = torch.Generator().manual_seed(SD_SEED)
    wave = (0.1 * torch.randn(1, L, generator=g)).cuda()
    mel = lm(wave)
    audio = voc(mel)
    assert mel.shape == (1, 80, lm.frames(L)) and audio.shape == (1, lm.frames(L) * 256)
    assert bool(torch.isfinite(audio).all())
