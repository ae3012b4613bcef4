"""The native Vocos vocoder at the sizes and configs where its kernels change: every GEMM tile path, the handle's
non-default configs, and the row limit of one launch.

The vocoder runs each GEMM over all R = B * T flattened rows as one item (engine_vocos.cpp), so gemm() (engine.cpp)
picks the tile from R: 256 x 256 BIG tiles when cout % 256 == 0 and ceil(R / 256) * cout / 256 >= big_min_blocks
(192), 64-frame T64 tiles for EPI_F32 when ceil(R / 128) * cout / 128 <= small_tiles (256), T128 otherwise; the
depthwise conv + LayerNorm runs 4 frames per wave from R >= 8192 (launch_voc_dwconv_ln).  At the default config
(C = 512, F = 1536, head cout 2 * 1152) that gives (tile_of() below restates it; test_tile_table_* pins it):

    GEMM / kernel                  R <= 900   first switch        second switch
    head     (EPI_F32,  cout 2304)  T64        T128 from R > 1792  BIG from R > 5376
    embed    (EPI_F32,  cout 512)   T64        T128 from R > 8192  BIG from R > 24320
    pwconv1  (EPI_GELU16, cout F)   T128       BIG from R > 7936   -
    pwconv2  (EPI_RESGATE, cout 512) T128      BIG from R > 24320  -
    dwconv + LayerNorm              R1         R4 from R >= 8192   -

    R = B x T            head   embed  pwconv1  pwconv2  dwconv
    3000  = 3 x 1000     T128   T64    T128     T128     R1
    6000  = 6 x 1000     BIG    T64    T128     T128     R1
    9009  = 9 x 1001     BIG    T128   BIG      T128     R4    (T odd: 4-frame groups straddle item ends)
    32000 = 32 x 1000    BIG    BIG    BIG      BIG      R4    (the bench shape)

The fp64 oracle runs only for the first, a middle and the last utterance of each batch (utterances are independent).
Gates as in test_gpu_vocos.py, relative to max|ref| of the utterance.
"""
import functools
import os
import types

import numpy as np
import pytest
import torch

from oracle import vocos_oracle as vo
from oracle.make_golden_vocos import CONFIG_CASES, CONFIGS, SD_SEED

TOL_AUDIO = {"f16": 1e-3, "bf16": 1e-2}
TOL_HIDDEN = {"f16": 1.5e-3, "bf16": 8e-3}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocos_outputs.npz")

# gemm() constants (engine_internal.h: big_min_blocks, small_tiles) and launch_voc_dwconv_ln's switch
BIG_MIN_BLOCKS, SMALL_TILES, DW_R4_ROWS, HEAD_COUT = 192, 256, 8192, 2 * 1152


def tile_of(R, cout, epi):
    """gemm()'s tile for a taps = 1 launch over R rows as one item (conc = 1, no split-K: cout != 256)."""
    t128, t256 = -(-R // 128), -(-R // 256)
    fills = t256 * 256 * 10 <= t128 * 128 * 11
    if cout % 256 == 0 and fills and t256 * (cout // 256) >= BIG_MIN_BLOCKS:
        return "BIG"
    return "T64" if epi == "F32" and t128 * (cout // 128) <= SMALL_TILES else "T128"


def vocoder_tiles(R, F=1536):
    return dict(head=tile_of(R, HEAD_COUT, "F32"), embed=tile_of(R, 512, "F32"), pwconv1=tile_of(R, F, "GELU16"),
                pwconv2=tile_of(R, 512, "RESGATE"), dwconv="R4" if R >= DW_R4_ROWS else "R1")


# (B, T) -> the tiles of the docstring table
TILE_BATCHES = {(3, 1000): ("T128", "T64", "T128", "T128", "R1"), (6, 1000): ("BIG", "T64", "T128", "T128", "R1"),
                (9, 1001): ("BIG", "T128", "BIG", "T128", "R4"), (32, 1000): ("BIG", "BIG", "BIG", "BIG", "R4")}


def test_tile_table_matches_gemm_rules():
    """The docstring table: its switch points and the tiles each tested batch runs (no GPU needed)."""
    def first(pred):
        return next(R for R in range(1, 40000) if pred(R))
    assert first(lambda R: tile_of(R, HEAD_COUT, "F32") != "T64") == 1793
    assert first(lambda R: tile_of(R, HEAD_COUT, "F32") == "BIG") == 5377
    assert first(lambda R: tile_of(R, 512, "F32") != "T64") == 8193
    assert first(lambda R: tile_of(R, 512, "F32") == "BIG") == 24321
    assert first(lambda R: tile_of(R, 1536, "GELU16") == "BIG") == 7937
    assert first(lambda R: tile_of(R, 512, "RESGATE") == "BIG") == 24321
    assert vocoder_tiles(900) == dict(head="T64", embed="T64", pwconv1="T128", pwconv2="T128", dwconv="R1")
    seen = set()
    for (B, T), want in TILE_BATCHES.items():
        got = vocoder_tiles(B * T)
        assert tuple(got.values()) == want, (B, T)
        seen |= set(got.items())
    # together the batches run every tile each kernel can take at this config
    assert seen >= {("head", "T128"), ("head", "BIG"), ("embed", "T64"), ("embed", "T128"), ("embed", "BIG"),
                    ("pwconv1", "T128"), ("pwconv1", "BIG"), ("pwconv2", "T128"), ("pwconv2", "BIG"),
                    ("dwconv", "R1"), ("dwconv", "R4")}


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
    return vo.make_mel(B, T, seed, M)


@functools.lru_cache(maxsize=None)
def _oracle(fields, B, T, seed, item):
    """fp64 hidden (T, C) and audio (T * 512) of utterance `item` of make_mel(B, T, seed)."""
    cfg = vo.vocos_config(**dict(fields))
    sd = _state_dict(fields)
    hid = vo.backbone_forward(sd, _mel(B, T, seed, cfg.input_channels)[item:item + 1], cfg)
    return hid[0], vo.head_forward(sd, hid, cfg)[0]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _run(voc, mel_np, capture):
    eng = voc.engine()
    eng.debug_capture(capture)
    try:
        audio = voc(torch.from_numpy(mel_np).cuda())
        hid = eng.debug_fetch("voc.hidden").reshape(mel_np.shape[0], mel_np.shape[2], -1) if capture else None
    finally:
        eng.debug_capture(False)
    return audio, hid


@pytest.fixture(scope="module", params=["f16", "bf16"])
def voc(request):
    return _vocoder({}, request.param)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", list(TILE_BATCHES), ids=[f"R{B * T}" for B, T in TILE_BATCHES])
def test_tile_paths_vs_oracle(voc, B, T):
    """Each batch size of the docstring table against the oracle (first, middle, last utterance), and each of those
    utterances run alone (a smaller R: other tiles) against the same utterance inside the batch."""
    dt, seed = voc.operand_dtype, 100 + B
    mel = _mel(B, T, seed)
    audio, hid = _run(voc, mel, capture=True)
    for i in (0, B // 2, B - 1):
        ref_h, ref_a = _oracle((), B, T, seed, i)
        eh, ea = _rel(hid[i], ref_h), _rel(audio[i].cpu().numpy(), ref_a)
        solo = voc(torch.from_numpy(mel[i:i + 1]).cuda())[0]
        es = 0.0 if torch.equal(solo, audio[i]) else _rel(solo.cpu().numpy(), audio[i].cpu().numpy())
        print(f"{dt} R={B * T} item {i}: hidden {eh:.2e} audio {ea:.2e} solo-vs-batch {es:.2e}")
        assert eh < TOL_HIDDEN[dt] and ea < TOL_AUDIO[dt], (i, eh, ea)
        assert es < 1e-6, (i, es)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [64, 65, 129])
def test_tile_edge_lengths_vs_oracle(voc, T):
    """Lengths at the edges of the im2col kernel's 64-frame tiles (a full tile, one frame past it, two tiles plus one),
    two utterances each, against the oracle (pinned to the reference by tests/test_oracle_golden.py; T = 1 and 2 are
    checked against the reference's own outputs in test_gpu_vocos.py)."""
    dt, B, seed = voc.operand_dtype, 2, 300 + T
    audio, hid = _run(voc, _mel(B, T, seed), capture=True)
    for i in range(B):
        ref_h, ref_a = _oracle((), B, T, seed, i)
        eh, ea = _rel(hid[i], ref_h), _rel(audio[i].cpu().numpy(), ref_a)
        print(f"{dt} T={T} item {i}: hidden {eh:.2e} audio {ea:.2e}")
        assert eh < TOL_HIDDEN[dt] and ea < TOL_AUDIO[dt], (i, eh, ea)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(CONFIG_CASES))
def test_configs_match_reference_fixtures(name, dtype):
    """The non-default configs of the fixture (input_channels 64 / 192, intermediate_dim 1024 / 2048, 3 / 1 layers)
    against the REAL reference module's outputs."""
    gold = np.load(GOLD)
    cname, B, T, seed = CONFIG_CASES[name]
    fields = CONFIGS[cname]
    voc = _vocoder(fields, dtype)
    audio, hid = _run(voc, _mel(B, T, seed, fields["input_channels"]), capture=True)
    eh, ea = _rel(hid, gold[name + ".hidden"]), _rel(audio.cpu().numpy(), gold[name + ".audio"])
    print(f"{dtype} {name}: hidden {eh:.2e} audio {ea:.2e}")
    assert eh < TOL_HIDDEN[dtype] and ea < TOL_AUDIO[dtype]


# name -> (VocosConfig fields, B, T, items checked)
ORACLE_CONFIGS = {
    "f256": (dict(intermediate_dim=256), 2, 300, (0, 1)),
    "f1280": (dict(intermediate_dim=1280), 10, 1000, (0, 9)),      # pwconv1: five 256-wide tiles, BIG (40 x 5 >= 192)
    "l12": (dict(num_layers=12), 2, 300, (0, 1)),
    "m192_t130": (dict(input_channels=192, intermediate_dim=2048, num_layers=1), 2, 130, (0, 1)),   # 55 KB im2col tile, 3 tiles
    "m64_t129": (dict(input_channels=64, intermediate_dim=1024, num_layers=3), 3, 129, (0, 2)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(ORACLE_CONFIGS))
def test_configs_vs_oracle(name, dtype):
    fields, B, T, items = ORACLE_CONFIGS[name]
    key, seed = tuple(sorted(fields.items())), 200 + B
    voc = _vocoder(fields, dtype)
    audio, hid = _run(voc, _mel(B, T, seed, vo.vocos_config(**fields).input_channels), capture=True)
    for i in items:
        ref_h, ref_a = _oracle(key, B, T, seed, i)
        eh, ea = _rel(hid[i], ref_h), _rel(audio[i].cpu().numpy(), ref_a)
        print(f"{dtype} {name} item {i}: hidden {eh:.2e} audio {ea:.2e}")
        assert eh < TOL_HIDDEN[dtype] and ea < TOL_AUDIO[dtype], i


def _check_items(voc, key, B, T, seed, items, label):
    """Runs the whole batch without debug capture; audio of `items` against the oracle."""
    mel = _mel(B, T, seed, vo.vocos_config(**dict(key)).input_channels)
    audio = voc(torch.from_numpy(mel).cuda())
    torch.cuda.synchronize()
    bad = []
    for i in items:
        ea = _rel(audio[i].cpu().numpy(), _oracle(key, B, T, seed, i)[1])
        print(f"{voc.operand_dtype} {label} item {i}: audio {ea:.2e}")
        if not ea < TOL_AUDIO[voc.operand_dtype]:
            bad.append((i, ea))
    del audio
    torch.cuda.empty_cache()
    assert not bad, bad


@pytest.mark.gpu
def test_row_limit_intermediate_4096():
    """R = 560,000 rows at intermediate_dim 4096: pwconv2's activation rows are 8 KiB, so a row offset formed in 32 bits
    inside the GEMM wraps from row 524,288 (item 524) on.  The forward runs such batches in chunks of whole utterances;
    every checked utterance matches the oracle, those beyond the wrap included."""
    need = 24 << 30
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need >> 30} GiB of free device memory, {free >> 30} GiB free")
    fields = dict(intermediate_dim=4096, num_layers=1)
    voc = _vocoder(fields, "f16")
    _check_items(voc, tuple(sorted(fields.items())), 560, 1000, 7, (0, 523, 524, 559), "F4096 R=560000")


@pytest.mark.gpu
def test_large_batch_beyond_grid_y():
    """B = 70,000 utterances of 2 frames: more items than a 65,535-row grid.y (im2col and overlap-add put B there)."""
    voc = _vocoder({}, "f16")
    _check_items(voc, (), 70000, 2, 8, (0, 35000, 65534, 65535, 65536, 69999), "B=70000 T=2")


@pytest.mark.gpu
def test_single_utterance_beyond_row_limit_is_refused():
    """One utterance longer than the 32-bit row bound (2^31 / (1536 * 2) rows at the default config) cannot be chunked:
    refused before any launch."""
    from stabletts_amd._lib import NativeError
    voc = _vocoder({}, "f16")
    T = (2 ** 31 - 1) // (1536 * 2) + 1
    with pytest.raises(NativeError, match="one utterance"):
        voc(torch.zeros(1, 128, T, device="cuda"))
