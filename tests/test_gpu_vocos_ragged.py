"""The native Vocos vocoder on ragged batches (Vocos.forward_ragged / st_vocos_forward_ragged): every utterance of a padded
batch vocoded at its own length.

The reference answer for utterance b is the fp64 oracle on that utterance ALONE, mel[b:b+1, :, :T_b] (the oracle is pinned
to the real module by tests/test_oracle_golden.py).  Gates are the vocoder's existing ones, relative to max|ref| of the
utterance: TOL_AUDIO / TOL_HIDDEN against the oracle, and 1e-6 for an utterance inside a ragged batch against the same
utterance through the dense call alone (another R may pick other GEMM tiles).  With every length equal to T the ragged
call runs the same arithmetic over the same rows as the dense one: bit equality.

The frames of the padded mel beyond an utterance's length are NaN wherever the test does not also need the dense call:
the ragged kernels must never read them.
"""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import vocos_oracle as vo
from oracle.make_golden_vocos import SD_SEED

TOL_AUDIO = {"f16": 1e-3, "bf16": 1e-2}
TOL_HIDDEN = {"f16": 1.5e-3, "bf16": 8e-3}
HOP = 512

# gemm() constants (engine_internal.h: big_min_blocks, small_tiles) and the depthwise kernel's switch (voc_dw_frames)
BIG_MIN_BLOCKS, SMALL_TILES, DW_R4_ROWS, HEAD_COUT = 192, 256, 8192, 2 * 1152


def tile_of(R, cout, epi):
    """gemm()'s tile for a taps = 1 launch over R rows as one item (conc = 1, no split-K: cout != 256)."""
    t128, t256 = -(-R // 128), -(-R // 256)
    fills = t256 * 256 * 10 <= t128 * 128 * 11
    if cout % 256 == 0 and fills and t256 * (cout // 256) >= BIG_MIN_BLOCKS:
        return "BIG"
    return "T64" if epi == "F32" and t128 * (cout // 128) <= SMALL_TILES else "T128"


def vocoder_tiles(R, F=1536):
    return (tile_of(R, HEAD_COUT, "F32"), tile_of(R, 512, "F32"), tile_of(R, F, "GELU16"), tile_of(R, 512, "RESGATE"),
            "R4" if R >= DW_R4_ROWS else "R1")


def _vocoder(fields, dtype):
    from stabletts_amd.vocos import Vocos
    cfg = vo.vocos_config(**fields)
    m = Vocos(types.SimpleNamespace(input_channels=cfg.input_channels, dim=cfg.dim, intermediate_dim=cfg.intermediate_dim,
                                    num_layers=cfg.num_layers),
              types.SimpleNamespace(n_fft=cfg.n_fft, hop_length=cfg.hop_length), operand_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _state_dict(tuple(sorted(fields.items()))).items()}, strict=True)
    return m.to("cuda:0")


@functools.lru_cache(maxsize=None)
def _state_dict(fields):
    return vo.make_vocos_state_dict(SD_SEED, vo.vocos_config(**dict(fields)))


@functools.lru_cache(maxsize=None)
def _mel(B, T, seed, M=128):
    mel = vo.make_mel(B, T, seed, M)
    mel.setflags(write=False)
    return mel


@functools.lru_cache(maxsize=None)
def _oracle(fields, B, T, seed, item, length):
    """fp64 hidden (length, C) and audio (length * 512) of the first `length` frames of utterance `item` of _mel(B, T, seed), alone."""
    cfg = vo.vocos_config(**dict(fields))
    sd = _state_dict(fields)
    hid = vo.backbone_forward(sd, _mel(B, T, seed, cfg.input_channels)[item:item + 1, :, :length], cfg)
    return hid[0], vo.head_forward(sd, hid, cfg)[0]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _padded(mel_np, lengths, fill):
    """The batch on the device with the frames beyond each length set to `fill`."""
    mel = torch.from_numpy(np.array(mel_np)).cuda()
    for b, n in enumerate(lengths):
        mel[b, :, n:] = fill
    return mel


def _nan_padded(mel_np, lengths):
    """As _padded(.., nan), for many utterances: one masked fill."""
    mel = torch.from_numpy(np.array(mel_np)).cuda()
    t = torch.arange(mel.shape[2], device="cuda")[None, None, :]
    n = torch.as_tensor(lengths, device="cuda")[:, None, None]
    return mel.masked_fill(t >= n, float("nan"))


def _run_ragged(voc, mel, lengths, capture=False):
    """audio (B, T * 512) and, with capture, the packed hidden (sum(lengths), C)."""
    eng = voc.engine()
    eng.debug_capture(capture)
    try:
        audio = voc.forward_ragged(mel, lengths)
        hid = eng.debug_fetch("voc.hidden").reshape(sum(lengths), -1) if capture else None
    finally:
        eng.debug_capture(False)
    return audio, hid


def _check_item(dt, audio, hid, offsets, lengths, b, ref, label):
    """Utterance b against its oracle (hidden only when captured); its tail must be exactly zero."""
    ref_h, ref_a = ref
    n = lengths[b]
    ea = _rel(audio[b, :n * HOP].cpu().numpy(), ref_a)
    eh = _rel(hid[offsets[b]:offsets[b] + n], ref_h) if hid is not None else 0.0
    print(f"{dt} {label} item {b} (T_b = {n}): hidden {eh:.2e} audio {ea:.2e}")
    assert eh < TOL_HIDDEN[dt] and ea < TOL_AUDIO[dt], (b, eh, ea)
    assert not audio[b, n * HOP:].any(), b


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).tolist()


@pytest.fixture(scope="module", params=["f16", "bf16"])
def voc(request):
    return _vocoder({}, request.param)


@pytest.fixture(scope="module")
def voc_f4096():
    return _vocoder(dict(intermediate_dim=4096, num_layers=1), "f16")


# ---------------------------------------------------------------- 1. padding contaminates, ragged does not
@pytest.mark.gpu
def test_padding_contaminates_dense_not_ragged(voc):
    dt, lengths, T, seed = voc.operand_dtype, [130, 70], 130, 41
    mel_np = _mel(2, T, seed)
    mel = _padded(mel_np, lengths, 0.0)
    ref = [_oracle((), 2, T, seed, b, lengths[b]) for b in range(2)]
    dense = voc(mel)
    last = slice(69 * HOP, 70 * HOP)        # item 1's last frame
    ed = float(np.abs(dense[1, last].cpu().numpy() - ref[1][1][last]).max() / np.abs(ref[1][1]).max())
    print(f"{dt} dense call on the zero-padded batch, item 1 last frame: {ed:.2e}")
    assert ed > 1e-2, ed
    audio, hid = _run_ragged(voc, mel, lengths, capture=True)
    assert audio.shape == (2, T * HOP)
    for b in range(2):
        _check_item(dt, audio, hid, _offsets(lengths), lengths, b, ref[b], "ragged")
    assert torch.equal(audio[1, 70 * HOP:], torch.zeros_like(audio[1, 70 * HOP:]))


# ---------------------------------------------------------------- 2. same arithmetic as the dense path
@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(2, 65), (9, 1001)], ids=["R130", "R9009"])
def test_equal_lengths_are_bitwise_the_dense_call(voc, B, T):
    """(9, 1001) runs the 4-frames-per-wave depthwise kernel with groups that end at item ends."""
    mel = torch.from_numpy(np.array(_mel(B, T, 50 + B))).cuda()
    dense = voc(mel)
    ragged = voc.forward_ragged(mel, [T] * B)
    assert torch.equal(ragged, dense)
    assert torch.equal(voc.forward_ragged(mel, torch.full((B,), T, dtype=torch.int32, device="cuda")), dense)


# ---------------------------------------------------------------- 3. tile and window edges
@pytest.mark.gpu
def test_edge_lengths_vs_oracle_and_solo(voc):
    """Lengths 1..4: the overlap-add's clamp and the +-3 window; 63 / 64 / 65 / 129: the im2col kernel's 64-frame tiles."""
    dt, lengths, T, seed = voc.operand_dtype, [1, 2, 3, 4, 63, 64, 65, 129, 7], 129, 42
    B = len(lengths)
    mel_np = _mel(B, T, seed)
    audio, hid = _run_ragged(voc, _padded(mel_np, lengths, float("nan")), lengths, capture=True)
    off = _offsets(lengths)
    for b, n in enumerate(lengths):
        _check_item(dt, audio, hid, off, lengths, b, _oracle((), B, T, seed, b, n), "edges")
        solo = voc(torch.from_numpy(np.array(mel_np[b:b + 1, :, :n])).cuda())[0]
        got = audio[b, :n * HOP]
        es = 0.0 if torch.equal(solo, got) else _rel(got.cpu().numpy(), solo.cpu().numpy())
        print(f"{dt} edges item {b}: ragged-vs-solo {es:.2e}")
        assert es < 1e-6, (b, es)


# ---------------------------------------------------------------- 4. every tile path with ragged lengths
def _odd_lengths(n, lo, step):
    return [lo + step * i for i in range(n)]        # lo odd, step even: odd and distinct


# name -> (lengths, the tiles (head, embed, pwconv1, pwconv2, dwconv) their sum runs: the R classes of test_gpu_vocos_shapes.py)
RAGGED_TILE_BATCHES = {
    "R3": (_odd_lengths(3, 971, 30), ("T128", "T64", "T128", "T128", "R1")),
    "R6": (_odd_lengths(6, 951, 20), ("BIG", "T64", "T128", "T128", "R1")),
    "R9": (_odd_lengths(9, 961, 10), ("BIG", "T128", "BIG", "T128", "R4")),
    # one frame between two long utterances
    "R32": (_odd_lengths(15, 941, 8) + [1] + _odd_lengths(16, 1061, 6), ("BIG", "BIG", "BIG", "BIG", "R4")),
}


def test_ragged_tile_batches_fall_in_their_classes():
    for name, (lengths, want) in RAGGED_TILE_BATCHES.items():
        assert vocoder_tiles(sum(lengths)) == want, (name, sum(lengths))
        assert len(set(lengths)) == len(lengths) and all(n % 2 == 1 for n in lengths), name
    lengths = RAGGED_TILE_BATCHES["R32"][0]
    assert lengths[15] == 1 and lengths[14] > 900 and lengths[16] > 900


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RAGGED_TILE_BATCHES))
def test_tile_paths_ragged_vs_oracle(voc, name):
    dt = voc.operand_dtype
    lengths, want = RAGGED_TILE_BATCHES[name]
    B, T, seed = len(lengths), max(lengths), 60 + len(lengths)
    assert vocoder_tiles(sum(lengths)) == want
    audio, hid = _run_ragged(voc, _nan_padded(_mel(B, T, seed), lengths), lengths, capture=True)
    off = _offsets(lengths)
    items = (0, 15, B - 1) if name == "R32" else (0, B // 2, B - 1)
    for b in items:
        _check_item(dt, audio, hid, off, lengths, b, _oracle((), B, T, seed, b, lengths[b]), name)
    assert not torch.isnan(audio).any()


# ---------------------------------------------------------------- 5. more utterances than grid-y
@pytest.mark.gpu
def test_more_utterances_than_grid_y():
    voc = _vocoder({}, "f16")
    B, T, seed = 70000, 3, 9
    lengths = [1 + b % 3 for b in range(B)]
    audio, _ = _run_ragged(voc, _nan_padded(_mel(B, T, seed), lengths), lengths)
    for b in (0, 35000, 65535, 65536, 69999):
        _check_item("f16", audio, None, None, lengths, b, _oracle((), B, T, seed, b, lengths[b]), "B=70000")
    assert not torch.isnan(audio).any()


# ---------------------------------------------------------------- 6. chunking on packed rows
F4096 = dict(intermediate_dim=4096, num_layers=1)
F4096_MAX_ROWS = (2 ** 31 - 1) // (4096 * 2)           # 262143 packed rows per chunk
F4096_LENGTHS = [800 + (b * 37) % 201 for b in range(300)]


def test_chunk_batch_needs_two_chunks():
    assert F4096_MAX_ROWS < sum(F4096_LENGTHS) <= 2 * F4096_MAX_ROWS
    assert min(F4096_LENGTHS) == 800 and max(F4096_LENGTHS) == 1000


@pytest.mark.gpu
def test_chunks_by_packed_rows(voc_f4096):
    """sum(lengths) exceeds the 262143-row bound of intermediate_dim 4096 (B * T = 300000 would, too, but the bound is on
    packed rows): two chunks; the last utterance of the first and the first of the second are checked."""
    lengths, B, T, seed = F4096_LENGTHS, 300, 1000, 10
    # workspace: 31488 bytes per packed row (im2col 1792, x 2048, h16 2 x 1024, u16 8192, head 9216, frames 8192)
    need = 12 << 30
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need >> 30} GiB of free device memory, {free >> 30} GiB free")
    off = _offsets(lengths)
    first2 = next(b for b in range(B) if off[b + 1] > F4096_MAX_ROWS)        # first utterance of chunk two
    key = tuple(sorted(F4096.items()))
    audio, _ = _run_ragged(voc_f4096, _nan_padded(_mel(B, T, seed), lengths), lengths)
    torch.cuda.synchronize()
    for b in (0, first2 - 1, first2, B - 1):
        _check_item("f16", audio, None, None, lengths, b, _oracle(key, B, T, seed, b, lengths[b]), "F4096 chunks")
    del audio
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 7. refusals
@pytest.mark.gpu
def test_refusals(voc_f4096):
    from stabletts_amd._lib import NativeError
    voc = _vocoder({}, "f16")
    mel = torch.zeros(3, 128, 10, device="cuda")
    with pytest.raises(NativeError, match=r"lengths\[1\] = 0 must be in \[1, T = 10\]"):
        voc.forward_ragged(mel, [10, 0, 5])
    with pytest.raises(NativeError, match=r"lengths\[2\] = 11 must be in \[1, T = 10\]"):
        voc.forward_ragged(mel, [10, 1, 11])
    with pytest.raises(NativeError, match="lengths has 2 entries, the batch has B = 3"):
        voc.forward_ragged(mel, [10, 5])
    with pytest.raises(ValueError, match="lengths is on meta"):
        voc.forward_ragged(mel, torch.empty(3, dtype=torch.int64, device="meta"))
    with pytest.raises(ValueError, match="integer tensor"):
        voc.forward_ragged(mel, torch.tensor([10.0, 5.0, 1.0]))
    with pytest.raises(ValueError, match="mel is on cpu"):
        voc.forward_ragged(mel.cpu(), [10, 5, 1])
    with pytest.raises(ValueError, match="input_channels"):
        voc.forward_ragged(mel[:, :64], [10, 5, 1])
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="inference-only"):     # (gpu tests run under no_grad)
        voc.forward_ragged(mel.clone().requires_grad_(True), [10, 5, 1])
    T = (2 ** 31 - 1) // (1536 * 2) + 1              # one utterance over the row bound of the default config
    with pytest.raises(NativeError, match="one utterance"):
        voc.forward_ragged(torch.zeros(1, 128, T, device="cuda"), [T])
    eng = voc_f4096.engine()                         # capture holds whole-batch tensors: a two-chunk batch is refused
    eng.debug_capture(True)
    try:
        with pytest.raises(NativeError, match="runs in chunks"):
            voc_f4096.forward_ragged(torch.zeros(300, 128, 1000, device="cuda"), F4096_LENGTHS)
    finally:
        eng.debug_capture(False)
    # the handle still works after every refusal
    assert torch.equal(voc.forward_ragged(mel, [10, 10, 10]), voc(mel))


@pytest.mark.gpu
def test_training_class_exposes_forward_ragged():
    """vocos_train.Vocos: the inference kernels under no_grad outside a differentiated call, a clear error inside one."""
    from stabletts_amd.vocos_train import Vocos
    cfg = vo.vocos_config()
    m = Vocos(types.SimpleNamespace(input_channels=cfg.input_channels, dim=cfg.dim, intermediate_dim=cfg.intermediate_dim,
                                    num_layers=cfg.num_layers), types.SimpleNamespace(n_fft=cfg.n_fft, hop_length=cfg.hop_length))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _state_dict(()).items()}, strict=True)
    m = m.to("cuda:0")
    mel = torch.from_numpy(np.array(_mel(2, 20, 43))).cuda()
    m.train()
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="no ragged form"):     # (gpu tests run under no_grad)
        m.forward_ragged(mel, [20, 9])
    m.eval()
    with torch.enable_grad():
        audio = m.forward_ragged(mel, [20, 9])
    assert not audio.requires_grad and not audio[1, 9 * HOP:].any()
    assert torch.equal(audio, _vocoder({}, "f16").forward_ragged(mel, [20, 9]))


# ---------------------------------------------------------------- 8. repeatable and stream-safe
@pytest.mark.gpu
def test_back_to_back_calls_keep_their_own_tables(voc):
    """Two calls with different length sets enqueued with no synchronisation between them (the second refills a table
    slot while the first may still run): each is bitwise its own single-call result."""
    B, T = 6, 400
    mel = torch.from_numpy(np.array(_mel(B, T, 44))).cuda()
    la, lb = [400, 1, 399, 64, 200, 37], [5, 400, 2, 333, 65, 128]
    ref_a = voc.forward_ragged(mel, la).clone()
    torch.cuda.synchronize()
    ref_b = voc.forward_ragged(mel, lb).clone()
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):                    # six calls: wraps the four slots
        outs.append((voc.forward_ragged(mel, la), voc.forward_ragged(mel, lb)))
    torch.cuda.synchronize()
    for a, b in outs:
        assert torch.equal(a, ref_a) and torch.equal(b, ref_b)
    assert not torch.equal(ref_a, ref_b)
