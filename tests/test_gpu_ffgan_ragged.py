"""The native FireflyGAN vocoder on ragged batches (FireflyGANBase.forward_ragged / st_ffgan_forward_ragged) on a real MI355X: every
utterance of a padded batch vocoded at its own length, every activation between mel and audio packed.

The reference answer for utterance b is the float64 restatement (tests/ffgan_restatement.py) on that utterance ALONE,
mel[b:b+1, :, :n_b].  The gate is the vocoder's existing one per compared tensor (tests/ffgan_checks.py): e_native <= 2 * e_emul and
e_emul < 2e-2, every pair printed (profiles/ffgan_ragged_parity.txt holds one run).  A head tile of the ragged call runs the
arithmetic of the dense call on its utterance alone, and the encoder's row kernels and GEMMs are per row, so wherever the packed
row count and the single utterance select the same GEMM tile (R <= 643 here: stem T64, pwconv T128 -- tile_of of
tests/test_gpu_ffgan_configs.py) the ragged audio is BITWISE the dense call's on that utterance alone.

The frames of the device mel beyond an utterance's length are NaN wherever the test does not also run the dense call: the ragged
kernels must never read them, and one NaN in an output shows that they did.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import ffgan_restatement as R
from tests.ffgan_checks import CONFIGS, build, gate
from tests.test_gpu_ffgan_configs import tile_of

DTYPES = ["f16", "bf16"]

# test 1: the longest is not first, T = 40 exceeds every length, 1- and 2-frame utterances sit between longer ones, and the level
# lengths (4 n and 8 n in "small") fall on both sides of 64, 128 and 256
EDGE_LENGTHS = [33, 1, 16, 17, 2, 32, 31, 15]
EDGE_BATCH = (8, 40, 41)                    # make_mel(B, T, M, seed)
EDGE_CONFIGS = ["small", "deep16", "four_by_four", "rates_6_10", "rates_16_12", "one_pair_k1", "wide_head", "mels192_narrowing"]
# test 2: conv_pre and ups[0] across one and two 128-frame tiles with a short neighbour
LEVEL0_BATCHES = {"T130": ((4, 130, 43), [127, 129, 1, 128]), "T260": ((3, 260, 44), [257, 3, 256])}


# ---------------------------------------------------------------- shared, made once, never written to
_models = {}


def model(name, dt):
    if (name, dt) not in _models:
        _models[(name, dt)] = build(R.DEFAULT if name == "default" else CONFIGS[name], dt)[0]
    return _models[(name, dt)]


def config(name):
    return R.DEFAULT if name == "default" else CONFIGS[name]


@functools.lru_cache(maxsize=None)
def _sd(name):
    return R.make_state_dict(config(name), R.SEED)


@functools.lru_cache(maxsize=None)
def _mel(name, B, T, seed):
    return R.make_mel(B, T, config(name)["backbone"]["input_channels"], seed)


def _three(out):
    return {n: out[n] for n in ("audio", "encoder", "pre_tanh")}


@functools.lru_cache(maxsize=None)
def _ref(name, B, T, seed, b, n):
    """float64 restatement of the first n frames of utterance b of _mel(name, B, T, seed), alone."""
    return _three(R.forward(_sd(name), config(name), _mel(name, B, T, seed)[b:b + 1, :, :n]))


@functools.lru_cache(maxsize=None)
def _e_emul(name, B, T, seed, b, n, dt):
    ref = _ref(name, B, T, seed, b, n)
    em = R.forward(_sd(name), config(name), _mel(name, B, T, seed)[b:b + 1, :, :n], dt, dt)
    return {k: R.rel_max(em[k], ref[k]) for k in ref}


def nan_padded(mel, lengths, fill=float("nan")):
    """The batch on the device with the frames beyond each length set to `fill`."""
    mel = mel.cuda()
    t = torch.arange(mel.shape[2], device="cuda")[None, None, :]
    n = torch.as_tensor(lengths, device="cuda")[:, None, None]
    return mel.masked_fill(t >= n, fill)


def run_ragged(m, mel, lengths, capture=False):
    """audio (B, T * hop) on the device and, with capture, the packed encoder (sum, D) and pre_tanh (sum * hop) as float64."""
    eng = m.engine()
    eng.debug_capture(capture)
    try:
        audio = m.forward_ragged(mel, lengths)
        torch.cuda.synchronize()
        enc = pre = None
        if capture:
            D = m.config["backbone"]["dims"][-1]
            enc = torch.from_numpy(eng.debug_fetch("ffgan.encoder").astype(np.float64)).view(sum(lengths), D)
            pre = torch.from_numpy(eng.debug_fetch("ffgan.pre_tanh").astype(np.float64))
            assert pre.numel() == sum(lengths) * m.hop_length
    finally:
        eng.debug_capture(False)
    return audio, enc, pre


def gate_items(name, dt, batch, lengths, audio, enc, pre, hop, items=None, label=""):
    """Every utterance (or `items`) against its own restatement; the tail of its audio must be exactly zero."""
    B, T, seed = batch
    off = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    assert audio.shape == (B, T * hop)
    a64 = audio.double().cpu()
    for b in (range(B) if items is None else items):
        n = lengths[b]
        got = {"audio": a64[b:b + 1, :n * hop]}
        names = ("audio",)
        if enc is not None:
            got["encoder"] = enc[off[b]:off[b] + n].t()[None]
            got["pre_tanh"] = pre[off[b] * hop:(off[b] + n) * hop][None]
            names = ("audio", "encoder", "pre_tanh")
        gate(f"{label or name} {dt} b{b} n{n}", got, _ref(name, B, T, seed, b, n), _e_emul(name, B, T, seed, b, n, dt), names)
        assert not a64[b, n * hop:].any(), (b, "tail")


def solo(m, mel, b, n):
    return m(mel[b:b + 1, :, :n].contiguous().cuda())[0]


# ---------------------------------------------------------------- 1. tile and halo edges
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", EDGE_CONFIGS)
def test_tile_and_halo_edges(name, dt):
    m = model(name, dt)
    mel = _mel(name, *EDGE_BATCH)
    audio, enc, pre = run_ragged(m, nan_padded(mel, EDGE_LENGTHS), EDGE_LENGTHS, capture=True)
    gate_items(name, dt, EDGE_BATCH, EDGE_LENGTHS, audio, enc, pre, m.hop_length)
    for b, n in enumerate(EDGE_LENGTHS):      # bitwise the dense call on the utterance alone (test 4)
        assert torch.equal(audio[b, :n * m.hop_length], solo(m, mel, b, n)), b


# ---------------------------------------------------------------- 2. level-0 tile edges
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", list(LEVEL0_BATCHES))
def test_level0_tile_edges(case, dt):
    batch, lengths = LEVEL0_BATCHES[case]
    m = model("small", dt)
    mel = _mel("small", *batch)
    audio, enc, pre = run_ragged(m, nan_padded(mel, lengths), lengths, capture=True)
    gate_items("small", dt, batch, lengths, audio, enc, pre, m.hop_length, label=f"small {case}")
    for b, n in enumerate(lengths):
        assert torch.equal(audio[b, :n * m.hop_length], solo(m, mel, b, n)), b


def test_bitwise_batches_select_one_gemm_tile():
    """Tests 1 and 2 compare bit for bit with single utterances: their packed row counts and every single length run the same
    GEMM tiles (no device needed; the widest encoder here is 768)."""
    for lengths in [EDGE_LENGTHS] + [ls for _, ls in LEVEL0_BATCHES.values()]:
        assert sum(lengths) <= 643
        for C in (128, 256, 640, 768):
            for r in lengths + [sum(lengths)]:
                assert (tile_of(r, C, "F32"), tile_of(r, 4 * C, "GELU16"), tile_of(r, C, "RESGATE")) == ("T64", "T128", "T128"), (r, C)


# ---------------------------------------------------------------- 3. padding contaminates the dense call, not the ragged one
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
def test_padding_contaminates_dense_not_ragged(dt):
    batch, lengths = (4, 40, 41), [40, 17, 1, 33]
    m = model("small", dt)
    hop = m.hop_length
    mel = nan_padded(_mel("small", *batch), lengths, 0.0)
    dense = m(mel).double().cpu()
    for b in (1, 2, 3):
        n = lengths[b]
        err = R.rel_max(dense[b:b + 1, :n * hop], _ref("small", *batch, b, n)["audio"])
        print(f"ffgan_ragged dense call on the zero-padded batch, {dt} item {b} (n = {n}): {err:.3e} of max |audio|")
        assert err > 0.1, (b, err)
    audio, enc, pre = run_ragged(m, mel, lengths, capture=True)
    gate_items("small", dt, batch, lengths, audio, enc, pre, hop, label="small padded0")


# ---------------------------------------------------------------- 4. bitwise conditions
@pytest.mark.gpu
@pytest.mark.parametrize("name,dt,B,T", [("default", "f16", 3, 9), ("deep16", "bf16", 3, 40), ("deep16", "f16", 3, 40)])
def test_equal_lengths_are_bitwise_the_dense_call(name, dt, B, T):
    m = model(name, dt)
    mel = _mel(name, B, T, 77).cuda()
    dense = m(mel)
    ragged = m.forward_ragged(mel, [T] * B)
    assert torch.equal(ragged, dense)
    assert torch.equal(m.forward_ragged(mel, torch.full((B,), T, dtype=torch.int32, device="cuda")), dense)
    assert torch.equal(m.forward_ragged(mel, [T] * B), ragged)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
def test_an_utterance_does_not_depend_on_its_neighbours(dt):
    """The batch of test 1 permuted, and with every other utterance's mel and length changed: utterance b's audio stays bit for bit."""
    m = model("small", dt)
    hop = m.hop_length
    mel = _mel("small", *EDGE_BATCH)
    base, _, _ = run_ragged(m, nan_padded(mel, EDGE_LENGTHS), EDGE_LENGTHS)
    again, _, _ = run_ragged(m, nan_padded(mel, EDGE_LENGTHS), EDGE_LENGTHS)
    assert torch.equal(base, again)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    lp = [EDGE_LENGTHS[i] for i in perm]
    out, _, _ = run_ragged(m, nan_padded(mel[perm], lp), lp)
    for k, i in enumerate(perm):
        n = EDGE_LENGTHS[i]
        assert torch.equal(out[k, :n * hop], base[i, :n * hop]), (k, i)
        assert not out[k, n * hop:].any()
    other = _mel("small", 8, 40, 99).clone()
    keep = 5                                                # 32 frames, now after seven utterances of other mels and lengths
    other[keep] = mel[keep]
    lo = [40, 3, 29, 1, 18, EDGE_LENGTHS[keep], 40, 9]
    out, _, _ = run_ragged(m, nan_padded(other, lo), lo)
    n = EDGE_LENGTHS[keep]
    assert torch.equal(out[keep, :n * hop], base[keep, :n * hop])


@pytest.mark.gpu
def test_back_to_back_calls_keep_their_own_tables():
    """Calls with different length sets enqueued with no synchronisation between them (a later one refills a table slot while an
    earlier one may still run): each is bitwise its own single-call result.  Six calls wrap the four slots."""
    m = model("small", "f16")
    mel = _mel("small", 6, 300, 45).cuda()
    la, lb = [300, 1, 299, 64, 200, 37], [5, 300, 2, 233, 65, 128]
    ref_a = m.forward_ragged(mel, la).clone()
    torch.cuda.synchronize()
    ref_b = m.forward_ragged(mel, lb).clone()
    torch.cuda.synchronize()
    outs = [(m.forward_ragged(mel, la), m.forward_ragged(mel, lb)) for _ in range(3)]
    torch.cuda.synchronize()
    for a, b in outs:
        assert torch.equal(a, ref_a) and torch.equal(b, ref_b)
    assert not torch.equal(ref_a, ref_b)


# ---------------------------------------------------------------- 5. chunks
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
def test_more_utterances_than_one_grid(dt):
    """B = 65537 > the 65535 items of one grid: chunks of 65535 and 2 utterances (audio only: debug capture refuses a chunked batch).
    A single-chunk call with capture still works afterwards."""
    from stabletts_amd._lib import NativeError
    m = model("small", dt)
    batch = (65537, 2, 500)
    lengths = [2 - (b & 1) for b in range(batch[0])]
    mel = nan_padded(_mel("small", *batch), lengths)
    audio, _, _ = run_ragged(m, mel, lengths)
    assert not torch.isnan(audio).any()
    gate_items("small", dt, batch, lengths, audio, None, None, m.hop_length, items=(0, 65534, 65535, 65536), label="small B65537")
    eng = m.engine()
    eng.debug_capture(True)
    try:
        with pytest.raises(NativeError, match="runs in chunks"):
            m.forward_ragged(mel, lengths)
    finally:
        eng.debug_capture(False)
    del audio, mel
    torch.cuda.empty_cache()
    small, ls = (2, 5, 501), [3, 5]
    audio, enc, pre = run_ragged(m, nan_padded(_mel("small", *small), ls), ls, capture=True)
    gate_items("small", dt, small, ls, audio, enc, pre, m.hop_length, label="small after chunks")


def head_rows_per_chunk(cfg):
    """Packed rows whose head level tensors (three fp32, one 16-bit: 14 bytes per channel-sample of the widest level) fill 1 GiB."""
    h = cfg["head"]
    up, widest = 1, h["upsample_initial_channel"]
    for i, u in enumerate(h["upsample_rates"]):
        up *= u
        widest = max(widest, up * (h["upsample_initial_channel"] >> (i + 1)))
    return (1 << 30) // (widest * 14)


WS_LENGTHS = [1000, 640, 900, 777, 600, 850, 990, 701, 812, 933, 655, 760]


def test_workspace_batch_needs_two_chunks():
    rows = head_rows_per_chunk(R.DEFAULT)
    assert rows == 9362 and rows < sum(WS_LENGTHS) <= 2 * rows
    assert len(WS_LENGTHS) == 12 and min(WS_LENGTHS) >= 600 and max(WS_LENGTHS) <= 1000


@pytest.mark.gpu
def test_chunks_by_the_head_workspace():
    """sum(lengths) exceeds the packed rows whose head workspace is 1 GiB: two chunks.  The last utterance of the first and the first
    of the second against those utterances alone through the dense call -- the same head arithmetic, while the encoder's GEMMs may
    select another tile at another row count: the bound of test_a_batch_that_runs_in_chunks (tests/test_gpu_ffgan.py), 2e-3 of
    max |audio|.  A wrong chunk offset is off by order 1."""
    m = model("default", "f16")
    lengths, B, T, hop = WS_LENGTHS, 12, 1000, 512
    off = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    first2 = next(b for b in range(B) if off[b + 1] > head_rows_per_chunk(R.DEFAULT))
    mel = _mel("default", B, T, 91)
    audio = m.forward_ragged(nan_padded(mel, lengths), lengths)
    assert audio.shape == (B, T * hop) and bool(torch.isfinite(audio).all())
    for b in (first2 - 1, first2):
        n = lengths[b]
        alone = solo(m, mel, b, n)
        err = float((audio[b, :n * hop] - alone).abs().max() / alone.abs().max())
        print(f"ffgan_ragged chunks item {b} (n = {n}): max |in batch - alone| / max = {err:.3e}")
        assert err <= 2e-3, (b, err)
    for b, n in enumerate(lengths):
        assert not audio[b, n * hop:].any(), b
    del audio
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 6. text to waveform for a bucket
@pytest.mark.gpu
def test_text_to_waveform_for_a_bucket(tmp_path):
    """The native synthesise chain (text -> padded mel) into wrapper.forward_ragged with the mel lengths read from the alignment."""
    import oracle
    from oracle.weights import DecoderConfig, TextEncoderConfig
    from stabletts_amd.ffgan import FireflyGANBaseWrapper
    from stabletts_amd.model import StableTTS
    torch.manual_seed(11)
    tts = StableTTS(401, 128, 256, 1024, 4, 1, 2, 3, 0.1, 256)
    tts.encoder.load_state_dict(oracle.make_text_encoder_state_dict(2468, TextEncoderConfig(n_layers=1), ada_std=0.15))
    tts.decoder.estimator.load_state_dict(oracle.make_state_dict(1234, DecoderConfig(n_layers=2), ada_std=0.15))
    tts = tts.cuda().eval()
    path = str(tmp_path / "generator.ckpt")
    torch.save(R.make_state_dict(R.DEFAULT, R.SEED), path)
    voc = FireflyGANBaseWrapper(path).cuda()
    gen = torch.Generator().manual_seed(7)
    x = torch.randint(1, 401, (2, 12), generator=gen).cuda()
    y = torch.randn(2, 128, 40, generator=gen).cuda()
    torch.manual_seed(5)
    out = tts.synthesise(x, torch.tensor([12, 7]).cuda(), 2, temperature=0.8, y=y, length_scale=1.0, solver="euler", cfg=2.0)
    mel, attn = out["decoder_outputs"], out["attn"]
    B, _, T = mel.shape
    lengths = (attn.sum(dim=(1, 2)) > 0).sum(dim=-1)             # frames that some token is aligned to
    ls = lengths.tolist()
    assert max(ls) == T and 1 <= min(ls) < T, ls
    audio = voc.forward_ragged(mel, lengths)
    assert audio.shape == (B, T * 512) and audio.dtype == torch.float32 and bool(torch.isfinite(audio).all())
    for b, n in enumerate(ls):
        assert not audio[b, n * 512:].any(), b
        assert torch.equal(audio[b, :n * 512], voc(mel[b:b + 1, :, :n])[0]), b
    assert float(audio.std()) > 1e-3


# ---------------------------------------------------------------- 7. entry-point rules
@pytest.mark.gpu
def test_entry_point_rules():
    from stabletts_amd import _lib
    from stabletts_amd._lib import NativeError
    m = model("small", "f16")
    eng = m.engine()
    lib, h = eng.lib, eng.handle
    mel = _mel("small", 3, 10, 5).cuda()
    audio = torch.zeros(3, 10 * m.hop_length, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(NativeError, match=r"lengths\[1\] = 0 must be in \[1, T = 10\]"):
        m.forward_ragged(mel, [10, 0, 5])
    with pytest.raises(NativeError, match=r"lengths\[2\] = 11 must be in \[1, T = 10\]"):
        m.forward_ragged(mel, [10, 1, 11])
    with pytest.raises(NativeError, match="lengths has 2 entries, the batch has B = 3"):
        m.forward_ragged(mel, [10, 5])
    arr = (ctypes.c_int64 * 3)(10, 5, 1)
    call = lambda *a: lib.st_ffgan_forward_ragged(h, *a, ctypes.c_void_p(s))      # noqa: E731
    assert call(mel.data_ptr(), None, audio.data_ptr(), 3, 10) == -1 and b"null lengths" in lib.st_last_error(h)
    assert call(None, arr, audio.data_ptr(), 3, 10) == -1 and b"null tensor" in lib.st_last_error(h)
    assert call(mel.data_ptr(), arr, None, 3, 10) == -1 and b"null tensor" in lib.st_last_error(h)
    assert call(mel.data_ptr(), arr, audio.data_ptr(), 0, 10) == -1
    assert call(mel.data_ptr(), arr, audio.data_ptr(), 3, 0) == -1
    assert call(mel.data_ptr(), arr, audio.data_ptr(), 3, (1 << 20) + 1) == -1 and b"T too large" in lib.st_last_error(h)
    voc = _lib.Engine(0, 0, 0, 0, 0, 0, 0, "f16", 0, vocoder=dict(input_channels=128, dim=512, intermediate_dim=1536, num_layers=8, n_fft=2048, hop_length=512))
    with pytest.raises(NativeError, match="not a FireflyGAN vocoder"):          # a Vocos handle
        voc.ffgan_forward_ragged(mel, [10, 5, 1], audio, s)
    voc.close()
    with pytest.raises(NativeError, match="not a vocoder"):                     # ... and the Vocos entry on this handle
        eng.vocos_forward_ragged(mel, [10, 5, 1], audio, s)
    fresh = _lib.Engine(0, 0, 0, 0, 0, 0, 0, "f16", 0, ffgan=m._fields)
    with pytest.raises(NativeError, match="st_finalize"):                       # before the parameters are loaded
        fresh.ffgan_forward_ragged(mel, [10, 5, 1], audio, s)
    fresh.close()
    # the argument rules of forward
    with pytest.raises(ValueError, match="lengths is on meta"):
        m.forward_ragged(mel, torch.empty(3, dtype=torch.int64, device="meta"))
    with pytest.raises(ValueError, match="integer tensor"):
        m.forward_ragged(mel, torch.tensor([10.0, 5.0, 1.0]))
    with pytest.raises(ValueError, match="no CPU fallback"):
        m.forward_ragged(mel.cpu(), [10, 5, 1])
    with pytest.raises(ValueError, match="input_channels"):
        m.forward_ragged(torch.zeros(3, 128, 10, device="cuda"), [10, 5, 1])
    with torch.enable_grad():       # (GPU tests run under no_grad unless marked grad)
        with pytest.raises(NotImplementedError, match="inference-only"):
            m.forward_ragged(mel.clone().requires_grad_(True), [10, 5, 1])
        assert m.forward_ragged(mel, [10, 5, 1]).shape == audio.shape      # nothing asks for grad: legal in any grad mode
    assert m.forward_ragged(mel.clone().requires_grad_(True), [10, 5, 1]).shape == audio.shape
    # the handle still works after the rejected calls
    assert torch.equal(m.forward_ragged(mel, [10, 10, 10]), m(mel))
