"""The native FireflyGAN vocoder across the configurations st_create_ffgan accepts, and at the sizes where its kernels and its
host code take another path, on a real MI355X against float64 (tests/ffgan_checks.py: the gate e_native <= 2 e_emul with
e_emul < 2e-2 per compared tensor, every pair printed; profiles/ffgan_config_parity.txt holds one run).  Configurations are
R.small_config() with the fields of ffgan_checks.CONFIGS changed, weights make_state_dict(cfg, R.SEED).

  rates       upsample rates 6, 10, 12, 14 and 16: ffg_pack_conv_kernel's polyphase map r = co / Co, j = r + u / 2 - u (tap - 1), the
              u * Cout row layout (cout 192: CW 4, cout 160: CW 2) and launch_ffg_tile_bias
  resblocks   one resblock with one dilation and kernel 1 (the pair reads X and writes straight into the mean, mean_first and mean_scale
              in one launch, halo 0, K padded from 16 to 32 at the 16-channel level); 4 resblocks x 4 dilations with kernels 13, 9, 5, 3
              and halos 24, 24, 24, 25
  encoder     widths 640 .. 1024 (the kFfgNi register arrays of the row kernels with ni = 5 .. 8), 192 mel channels (55 KB im2col tile,
              GEMM K = 1344), a narrowing encoder (Dmax != D), eight stages, one stage
  wide head   head widths 1024 -> 512 -> 256: cin = 1024 and 512 (8 and 4 K-chunks per block), conv_post over 256 channels
  level 0     conv_pre (cin 256: two K-chunks, 16-bit input) and ups[0] run at level length T: T = 127, 128, 129 and 257 cross one and
              two 128-frame tiles there; the post kernel crosses several 256-sample tiles
  GEMM tiles  the encoder's GEMMs run over all R = B * T flattened rows as one item, so gemm() (engine.cpp) picks the tile from R:
              tile_of() below restates the rule, test_tile_table_matches_gemm_rules pins the table (no device needed)

                  GEMM (at dims (1024, 1024))              switch points
                  stem, downsample (EPI_F32, cout 1024)    T64 up to R = 4096, T128 from 4097, BIG from 12033
                  pwconv1 (EPI_GELU16, cout 4096)          T128 up to R = 2816, BIG from 2817
                  pwconv2 (EPI_RESGATE, cout 1024)         T128 up to R = 12032, BIG from 12033

                  R = B x T           stem, downsample   pwconv1   pwconv2
                  3000  = 6 x 500     T64                BIG       T128
                  4509  = 9 x 501     T128               BIG       T128
                  12100 = 11 x 1100   BIG                BIG       BIG        (pwconv1's T128 runs in every other case here: R <= 514)

  chunks      B = 65537 utterances of 2 frames: the 65535-item grid limit splits the batch into chunks of 65535 and 2
  fixture     the reference's own encoder and head at two further configurations (tests/golden/ffgan_config_outputs.npz)
"""
import os

import numpy as np
import pytest
import torch

from tests import ffgan_restatement as R
from tests.ffgan_checks import against_restatement, build, gate, run_captured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["f16", "bf16"]

# gemm() constants (engine_internal.h: big_min_blocks, small_tiles; st_create_ffgan changes neither)
BIG_MIN_BLOCKS, SMALL_TILES = 192, 256


def tile_of(R_, cout, epi):
    """gemm()'s tile for a taps = 1 launch over R_ rows as one item (conc = 1; an ffgan handle has no split-K planes)."""
    t128, t256 = -(-R_ // 128), -(-R_ // 256)
    fills = t256 * 256 * 10 <= t128 * 128 * 11
    if cout % 256 == 0 and fills and t256 * (cout // 256) >= BIG_MIN_BLOCKS:
        return "BIG"
    return "T64" if epi == "F32" and t128 * (cout // 128) <= SMALL_TILES else "T128"


def encoder_tiles(R_, C=1024):
    return dict(stem=tile_of(R_, C, "F32"), pwconv1=tile_of(R_, 4 * C, "GELU16"), pwconv2=tile_of(R_, C, "RESGATE"))


# (B, T) -> the tiles of the docstring table
TILE_BATCHES = {(6, 500): ("T64", "BIG", "T128"), (9, 501): ("T128", "BIG", "T128"), (11, 1100): ("BIG", "BIG", "BIG")}


def test_tile_table_matches_gemm_rules():
    """The docstring table: its switch points and the tiles each tested batch runs (no GPU needed)."""
    def first(pred):
        return next(r for r in range(1, 40000) if pred(r))
    assert first(lambda r: tile_of(r, 1024, "F32") != "T64") == 4097
    assert tile_of(4097, 1024, "F32") == "T128"
    assert first(lambda r: tile_of(r, 1024, "F32") == "BIG") == 12033
    assert first(lambda r: tile_of(r, 4096, "GELU16") == "BIG") == 2817
    assert first(lambda r: tile_of(r, 1024, "RESGATE") == "BIG") == 12033
    assert {tile_of(r, 4096, "GELU16") for r in range(1, 2817)} == {"T128"}
    assert {tile_of(r, 1024, "RESGATE") for r in range(1, 12033)} == {"T128"}
    seen = set()
    for (B, T), want in TILE_BATCHES.items():
        got = encoder_tiles(B * T)
        assert tuple(got.values()) == want, (B, T)
        seen |= set(got.items())
    # every other case of this file has R <= 514: the smallest path of each GEMM at its own widths
    assert encoder_tiles(2 * 257) == dict(stem="T64", pwconv1="T128", pwconv2="T128")
    seen |= set(encoder_tiles(2 * 13).items())      # wide_1024_896 at 2 x 13
    # together the batches run every tile each GEMM can take
    assert seen == {("stem", "T64"), ("stem", "T128"), ("stem", "BIG"), ("pwconv1", "T128"), ("pwconv1", "BIG"),
                    ("pwconv2", "T128"), ("pwconv2", "BIG")}


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,T", [("rates_6_10", 11), ("rates_14_2", 11), ("rates_16_12", 7)])
def test_upsample_rates(name, T, dt):
    against_restatement(name, dt, 2, T, 41)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,T", [("one_pair_k1", 21), ("four_by_four", 40)])
def test_resblock_shapes(name, T, dt):
    against_restatement(name, dt, 2, T, 41)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["mels192_narrowing", "wide_1024_896", "eight_stages", "one_stage"])
def test_encoder_shapes(name, dt):
    against_restatement(name, dt, 2, 13, 41)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
def test_wide_head(dt):
    against_restatement("wide_head", dt, 2, 9, 41)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T", [127, 128, 129, 257])
def test_level0_tile_edges(T, dt):
    against_restatement("small", dt, 2, T, 300 + T)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,T", list(TILE_BATCHES), ids=[f"R{B * T}" for B, T in TILE_BATCHES])
def test_encoder_gemm_tile_paths(B, T, dt):
    """The first, the middle and the last utterance of each batch of the docstring table against the restatement."""
    against_restatement("tile_paths", dt, B, T, 100 + B, items=(0, B // 2, B - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
def test_a_chunked_batch_against_float64(dt):
    """B = 65537 > the 65535 items of one grid: chunks of 65535 and 2.  The first item, the last item of the first chunk and both
    items of the second against the restatement of those four mels (audio only: debug capture is refused for chunked batches)."""
    against_restatement("small", dt, 65537, 2, 500, items=(0, 65534, 65535, 65536), capture=False)
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ffgan_config_outputs.npz")))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(R.REF_CASES))
def test_configs_match_the_reference_fixture(gold, name, dt):
    """The native module against the reference's own encoder and head (tools/make_golden_ffgan.py), e_emul from the fixture."""
    cfg, B, T, mel_seed = R.REF_CASES[name]
    m, _ = build(cfg, dt)
    got = run_captured(m, R.make_mel(B, T, cfg["backbone"]["input_channels"], mel_seed))
    ref = {n: torch.from_numpy(gold[f"{name}/{n}"]) for n in ("audio", "encoder", "pre_tanh")}
    em = gold[f"{name}/emul_{dt}"][0]
    gate(f"{name} {B}x{T} {dt}", got, ref, {"audio": em[0], "encoder": em[1], "pre_tanh": em[2]})
