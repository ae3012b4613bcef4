"""The native Vocos vocoder at backbone widths 768 and 1024 (12 and 16 channels per lane in the row kernels of vocos_kernels.hip;
768 is the width of the Vocos trainer's own generator, vocoders/vocos/config.py:21-26).

Reference: the float64 oracle (pinned to the real module at these widths by tests/test_vocos_dims_cpu.py).  Metric and gates are
those of tests/test_gpu_vocos.py / test_gpu_vocos_shapes.py: max |audio - ref| / max |ref| per utterance, 1e-3 with f16 operands
(1e-2 with bf16), at depths (1 - 2 layers) at which dim 512 passes that gate.  Every error is printed beside its gate.

The GEMMs run over the R = B * T flattened rows as one item, so gemm() (engine.cpp) picks the tile from R and cout
(test_gpu_vocos_shapes.tile_of restates the rule).  For cout = dim (embed: EPI_F32; pwconv2: EPI_RESGATE) the switches are

    cout 768:   T64 -> T128 above R = 5376 (43 x 6 > 256 tiles),  BIG above R = 16128 (64 x 3 >= 192 blocks)
    cout 1024:  T64 -> T128 above R = 4096 (33 x 8 > 256 tiles),  BIG above R = 12032 (48 x 4 >= 192 blocks)

and the depthwise conv + LayerNorm runs 4 frames per wave from R = 8192 rows at every width (voc_dw_frames).

The comparison of dim 512 with a library built from the parent commit (bitwise, dense and ragged, on the inputs of
tests/golden/vocos_outputs.npz) needs that second library, which a checkout does not hold: tools/vocos_dims_parity.py does it and
profiles/vocos_dims_parity.txt records it.

MEASURED on an MI355X (f16 unless said): dense cases 4.4e-04 .. 8.1e-04 at both widths, every tile path included; the trainer's
generator (12 layers) 6.06e-04 with f16 operands and about 1e-06 through the fp32 training forward.
"""
import numpy as np
import pytest
import torch

from oracle import vocos_oracle as vo
from tests import vocos_dims_cases as D
from tests.test_gpu_vocos_shapes import BIG_MIN_BLOCKS, DW_R4_ROWS, SMALL_TILES, TOL_AUDIO, _mel, _oracle, _rel, _vocoder, tile_of

pytestmark = pytest.mark.gpu
DIMS = [768, 1024]
HOP = 512


def _fields(dim, **over):
    return {**dict(input_channels=64, dim=dim, intermediate_dim=256, num_layers=2), **over}


def _key(fields):
    return tuple(sorted(fields.items()))


@pytest.fixture(scope="module")
def vocs():
    """(dim, dtype, config overrides) -> vocoder, built once per module."""
    made = {}

    def get(dim, dtype="f16", **over):
        k = (dim, dtype, _key(over))
        if k not in made:
            made[k] = _vocoder(_fields(dim, **over), dtype)
        return made[k]
    return get


def _check(voc, fields, B, T, seed, items, label):
    cfg = vo.vocos_config(**fields)
    dt = voc.operand_dtype
    audio = voc(torch.from_numpy(np.array(_mel(B, T, seed, cfg.input_channels))).cuda())
    assert audio.shape == (B, T * HOP) and torch.isfinite(audio).all()
    bad = []
    for i in items:
        ea = _rel(audio[i].cpu().numpy(), _oracle(_key(fields), B, T, seed, i)[1])
        print(f"{dt} dim {cfg.dim} {label} R={B * T} item {i}: audio {ea:.2e} (gate {TOL_AUDIO[dt]:.0e})")
        if not ea < TOL_AUDIO[dt]:
            bad.append((i, ea))
    assert not bad, bad
    return audio


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("B,T", [(1, 1), (2, 3), (3, 7), (2, 130)], ids=lambda v: str(v))
def test_dense_vs_oracle(vocs, dim, B, T):
    _check(vocs(dim), _fields(dim), B, T, 400 + B + T, range(B), "dense")


@pytest.mark.parametrize("dim", DIMS)
def test_dense_vs_oracle_bf16(vocs, dim):
    _check(vocs(dim, "bf16"), _fields(dim), 2, 130, 532, range(2), "dense")


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("over", [dict(intermediate_dim=2048), dict(input_channels=192)], ids=["F2048", "M192"])
def test_other_configs_vs_oracle(vocs, dim, over):
    _check(vocs(dim, **over), _fields(dim, **over), 2, 70, 440, range(2), "+".join(f"{k}={v}" for k, v in over.items()))


@pytest.mark.parametrize("dim", DIMS)
def test_four_frame_depthwise_path_and_its_tail(vocs, dim):
    """R = 3 x 2731 = 8193 rows: the first row count >= 8192 (where voc_dw_frames leaves 1 frame per wave, at every width) whose
    T is no multiple of 4 with more than one frame per utterance -- the last group of every utterance holds 3 frames.  Against
    the oracle, against each utterance alone (R = 2731: one frame per wave), and the ragged kernel at the same rows, bitwise."""
    B, T, seed = 3, 2731, 451
    assert B * T >= DW_R4_ROWS > (B - 1) * T and T % 4 == 3 and T < DW_R4_ROWS
    fields = _fields(dim, num_layers=1)
    voc = vocs(dim, num_layers=1)
    audio = _check(voc, fields, B, T, seed, (0, B - 1), "R4")
    mel = torch.from_numpy(np.array(_mel(B, T, seed, 64))).cuda()
    for i in (0, B - 1):
        solo = voc(mel[i:i + 1].contiguous())[0]
        es = 0.0 if torch.equal(solo, audio[i]) else _rel(solo.cpu().numpy(), audio[i].cpu().numpy())
        print(f"f16 dim {dim} R4 item {i}: one frame per wave (alone) vs four (batch) {es:.2e} (gate 1e-6)")
        assert es < 1e-6
    assert torch.equal(voc.forward_ragged(mel, [T] * B), audio)


# cout = dim: (B, T) just below and just above each switch of gemm()'s tile choice (module docstring)
TILE_EDGES = {768: [(21, 256), (19, 283), (126, 128), (127, 127)], 1024: [(32, 128), (17, 241), (94, 128), (21, 573)]}


def test_tile_edges_follow_gemms_rule():
    """The switch points from the rule (no GPU needed): each pair of TILE_EDGES straddles one."""
    def first(pred):
        return next(R for R in range(1, 40000) if pred(R))
    for dim, want in ((768, (5377, 16129)), (1024, (4097, 12033))):
        assert (SMALL_TILES // (dim // 128)) * 128 + 1 == want[0] and -(-BIG_MIN_BLOCKS // (dim // 256)) * 256 - 255 == want[1]
        assert first(lambda R: tile_of(R, dim, "F32") != "T64") == want[0]
        assert first(lambda R: tile_of(R, dim, "F32") == "BIG") == first(lambda R: tile_of(R, dim, "RESGATE") == "BIG") == want[1]
        rows = [B * T for B, T in TILE_EDGES[dim]]
        assert rows == [want[0] - 1, want[0], want[1] - 1, want[1]]
        assert [tile_of(R, dim, "F32") for R in rows] == ["T64", "T128", "T128", "BIG"]
        assert [tile_of(R, dim, "RESGATE") for R in rows] == ["T128", "T128", "T128", "BIG"]


@pytest.mark.parametrize("dim,B,T", [(d, B, T) for d in DIMS for B, T in TILE_EDGES[d]], ids=lambda v: str(v))
def test_gemm_tile_paths_vs_oracle(vocs, dim, B, T):
    _check(vocs(dim, num_layers=1), _fields(dim, num_layers=1), B, T, 460, (0, B - 1), "tiles")


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("lengths", [(130, 70, 1), (64, 65, 63)], ids=lambda v: "-".join(map(str, v)))
def test_ragged_is_bitwise_each_utterance_alone(vocs, dim, lengths):
    """The assertions of tests/test_gpu_vocos_ragged.py at the new widths: NaN in the padded frames is never read, every utterance
    is bitwise that utterance alone through the dense call (checked against the oracle by the tests above), the padded tail of
    the audio is zero, and equal lengths are bitwise the dense call."""
    voc, B, T = vocs(dim), len(lengths), max(lengths)
    mel_np = _mel(B, T, 470 + T, 64)
    mel = torch.from_numpy(np.array(mel_np)).cuda()
    t = torch.arange(T, device="cuda")[None, None, :]
    nan_mel = mel.masked_fill(t >= torch.as_tensor(lengths, device="cuda")[:, None, None], float("nan"))
    audio = voc.forward_ragged(nan_mel, list(lengths))
    assert audio.shape == (B, T * HOP) and torch.isfinite(audio).all()
    for b, n in enumerate(lengths):
        solo = voc(mel[b:b + 1, :, :n].contiguous())[0]
        assert torch.equal(audio[b, :n * HOP], solo), b
        assert not audio[b, n * HOP:].any(), b
    assert torch.equal(voc.forward_ragged(mel, [T] * B), voc(mel))


@pytest.mark.parametrize("dim", DIMS)
def test_two_runs_are_bitwise_equal(vocs, dim):
    voc = vocs(dim)
    mel = torch.from_numpy(np.array(_mel(3, 77, 481, 64))).cuda()
    a, b = voc(mel), voc(mel)
    assert torch.equal(a, b)
    assert torch.equal(voc.forward_ragged(mel, [77, 5, 40]), voc.forward_ragged(mel, [77, 5, 40]))


@pytest.mark.grad
def test_the_trainers_generator():
    """128 / 768 / 2048 / 12 at B = 1, T = 40.  Whether f16 operands stay inside 1e-3 through 12 layers at this width is a
    measurement (printed with the bar beside it; profiles/vocos_dims_parity.txt), not a gate: this case asserts that the output
    is finite and that the fp32 training forward of the same input is inside 1e-3."""
    from stabletts_amd.vocos_train import Vocos as TrainVocos
    from tests.test_gpu_vocos_training import _module
    cfg = vo.vocos_config(**D.TRAINER)
    sd = vo.make_vocos_state_dict(141, cfg)
    mel_np = vo.make_mel(1, 40, 491, 128)
    ref = vo.vocos_forward(sd, mel_np, cfg)
    mod = _module(cfg, sd, TrainVocos)
    mel = torch.from_numpy(mel_np).cuda()
    with torch.no_grad():
        a16 = mod.eval()(mel).cpu().numpy()
    with torch.enable_grad():
        a32 = mod.train()(mel).detach().cpu().numpy()
    e16, e32 = _rel(a16, ref), _rel(a32, ref)
    print(f"trainer's generator (128/768/2048/12, B=1 T=40): f16 inference {e16:.2e} (bar 1e-3, not asserted), fp32 training forward {e32:.2e} (gate 1e-3)")
    assert np.isfinite(a16).all() and np.isfinite(a32).all()
    assert e32 < 1e-3
