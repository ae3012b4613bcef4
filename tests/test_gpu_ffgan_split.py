"""The split-precision FireflyGAN vocoder (operand_dtype "f16_split" / "bf16_split") on a real MI355X against float64.

Accuracy gate, per compared tensor (audio, encoder, pre_tanh), e = max |. - float64| / max |float64| (tests/ffgan_split_checks.py):
    e_native <= e_emul_split + 4 * e_fp32      and      e_native < 1e-3 (the project's bar)
e_emul_split: the float64 restatement with split-rounded weights and inputs; e_fp32: the same restatement code in float32 on the CPU.
("bf16_split" runs four products in the encoder and three bf16 parts in the head, and is measured against the same PAIR emulation.)
Every pair is printed with its ratio to the bound; profiles/ffgan_split_parity.txt holds one run.  Whether the MFMA keeps the
subnormal lo halves of f16 is part of what the f16_split cases show: flushed, they would sit near 1e-4, far above the bound.
"""
import os

import numpy as np
import pytest
import torch

from tests import ffgan_restatement as R
from tests import ffgan_split_checks as S
from tests.ffgan_checks import NAMES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = ["f16_split", "bf16_split"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ffgan_outputs.npz")))


def _fixture_ref(gold, prefix):
    return {n: torch.from_numpy(gold[f"{prefix}/{n}"]) for n in NAMES}


# ---------------------------------------------------------------- 1, 7: the default configuration against the real module's fixture
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_default_config_matches_the_reference_fixture(gold, ci, dt):
    B, T = R.CASES[ci]
    S.against_restatement("default", dt, B, T, R.MEL_SEED + ci, ref=_fixture_ref(gold, f"{B}x{T}"))


@pytest.mark.parametrize("ci", [0, 1])
def test_split_is_20x_closer_than_f16_operands(gold, ci):
    """The same input through an "f16" handle and an "f16_split" handle of the same build (the CPU figures put the ratio above 100)."""
    B, T = R.CASES[ci]
    mel = R.make_mel(B, T, 128, R.MEL_SEED + ci).cuda()
    ref = gold[f"{B}x{T}/audio"]
    e = {dt: R.rel_max(S.model("default", dt)(mel).double().cpu(), ref) for dt in ("f16", "f16_split")}
    print(f"ffgan_split_discrimination default {B}x{T}: e_native f16 {e['f16']:.3e}   f16_split {e['f16_split']:.3e}   ratio {e['f16'] / e['f16_split']:.1f}")
    assert e["f16_split"] * 20 <= e["f16"], e


# ---------------------------------------------------------------- 2: frame-tile and halo edges
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 31, 33])
def test_frame_tile_edges(T, dt):
    """Level lengths 4 T and 8 T: below one halo (T = 1, 2), and on both sides of 64, 128 and 256 frames (the kernel's tile is 128)."""
    S.against_restatement("small", dt, 2, T, 300 + T)


@pytest.mark.parametrize("dt", DTS)
def test_the_16_channel_level(dt):
    """deep16: 64 -> 32 -> 16 channels, k = 11 at dilation 5: cin 64, 32 and 16, each one K chunk at or below the split chunk of 64."""
    S.against_restatement("deep16", dt, 2, 21, 41)


# ---------------------------------------------------------------- 3, 4: the reference's own modules at two further configurations
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["ref_b", "ref_a"])
def test_other_configurations_match_the_reference_fixture(name, dt):
    """ref_b: halo 25 (the largest patch: 178 rows in two planes, or in bf16's three -- 76 896 bytes, through the LDS opt-in), kernels 1
    and 13, a 1024-wide encoder whose pwconv2 re-reads the pair tensor of 4 C = 4096 values per half.  ref_a: 192 mel channels (stem K = 3 x 7 x 192), widths 768 and 640 (other GEMM tiles), rates 6 and 10."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ffgan_config_outputs.npz"))
    _, B, T, mel_seed = R.REF_CASES[name]
    S.against_restatement(name, dt, B, T, mel_seed, ref=_fixture_ref(gold, name))


# ---------------------------------------------------------------- 5: bitwise properties
@pytest.mark.parametrize("dt", DTS)
def test_runs_repeat_and_items_are_independent_bitwise(dt):
    for name, B, T, M in (("default", 3, 9, 128), ("deep16", 3, 40, 64)):
        m = S.model(name, dt)
        mel = R.make_mel(B, T, M, 77).cuda()
        a = m(mel)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, m(mel))
        for i in range(B):
            assert torch.equal(m(mel[i:i + 1].contiguous())[0], a[i]), (name, i)


@pytest.mark.parametrize("dt", DTS)
def test_ragged_call_is_each_utterance_alone_bitwise(dt):
    """Lengths (33, 17, 1, 33), NaN in the padded mel: every utterance bitwise that utterance alone, a zero tail; with equal lengths
    bitwise the dense call.  (84 packed rows and every single utterance select the same GEMM tiles.)"""
    m = S.model("small", dt)
    hop = m.hop_length
    lengths = [33, 17, 1, 33]
    mel = R.make_mel(4, 33, 64, 52).cuda()
    t = torch.arange(33, device="cuda")[None, None, :]
    padded = mel.masked_fill(t >= torch.as_tensor(lengths, device="cuda")[:, None, None], float("nan"))
    audio = m.forward_ragged(padded, lengths)
    assert audio.shape == (4, 33 * hop) and bool(torch.isfinite(audio).all())
    assert torch.equal(audio, m.forward_ragged(padded, lengths))
    for b, n in enumerate(lengths):
        alone = m(mel[b:b + 1, :, :n].contiguous())[0]
        assert torch.equal(audio[b, :n * hop], alone), b
        assert not bool(audio[b, n * hop:].any()), b
    assert torch.equal(m.forward_ragged(mel, [33] * 4), m(mel))
    d = S.model("default", dt)
    mel = R.make_mel(2, 9, 128, 53).cuda()
    assert torch.equal(d.forward_ragged(mel, [9, 9]), d(mel))
    r = d.forward_ragged(mel, [9, 4])
    assert torch.equal(r[1, :4 * 512], d(mel[1:2, :, :4].contiguous())[0]) and not bool(r[1, 4 * 512:].any())


# ---------------------------------------------------------------- 6: chunks by the head workspace
@pytest.mark.parametrize("dt", DTS)
def test_chunks_by_the_head_workspace(dt):
    """The split head keeps four fp32 tensors of the widest level: 16 bytes per channel-sample (14 with 16-bit operands), so
    T = 1000 at the default configuration is 8192 x 1000 x 16 = 131.1 MB per utterance and the 1 GiB bound holds 8 (not 9): B = 9 runs
    as 8 + 1.  The last item of the first chunk and the item of the second against those utterances alone; same bound as the default
    mode's test (2e-3 of max |audio|: the encoder's GEMMs may pick another tile for another row count); a wrong offset is off by order 1.
    Which chunking ran is pinned through the debug capture, which refuses a batch that runs in chunks: with capture on, 8 utterances run
    and 9 are refused, in the dense and in the ragged call (14 bytes would let 9 through); a default-mode handle runs the 9."""
    from stabletts_amd._lib import NativeError
    m = S.model("default", dt)
    assert (1 << 30) // (8192 * 1000 * 16) == 8 and (1 << 30) // (8192 * 1000 * 14) == 9
    mel = R.make_mel(9, 1000, 128, 91).cuda()
    audio = m(mel)
    assert audio.shape == (9, 512000) and bool(torch.isfinite(audio).all())
    ragged = m.forward_ragged(mel, [1000] * 9)
    for i in (7, 8):
        alone = m(mel[i:i + 1].contiguous())[0]
        for tag, got in (("dense", audio[i]), ("ragged", ragged[i])):
            err = float((got - alone).abs().max() / alone.abs().max())
            print(f"ffgan_split_chunks {dt} {tag} item {i}: max |in batch - alone| / max = {err:.3e}")
            assert err <= 2e-3, (tag, i, err)
    del ragged
    first8 = mel[:8].contiguous()
    for mod, refused in ((m, True), (S.model("default", "f16"), False)):
        eng = mod.engine()
        eng.debug_capture(True)
        try:
            got = mod(first8)                                                               # one chunk: runs with the capture on
            if mod is m:
                assert torch.equal(got, audio[:8])                                          # ... and is the first chunk of the nine
            assert mod.forward_ragged(first8, [1000] * 8).shape == (8, 512000)
            for call in (lambda: mod(mel), lambda: mod.forward_ragged(mel, [1000] * 9)):
                if refused:
                    with pytest.raises(NativeError, match="runs in chunks"):
                        call()
                else:
                    assert call().shape == (9, 512000)
        finally:
            eng.debug_capture(False)
    assert torch.equal(m(mel), audio)                                                       # the handle works after the refusals


# ---------------------------------------------------------------- 8: the wrapper
def test_text_to_waveform_through_the_wrapper(tmp_path):
    """The native synthesise chain (text -> mel) feeding FireflyGANBaseWrapper(path, operand_dtype="f16_split")."""
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
    voc = FireflyGANBaseWrapper(path, operand_dtype="f16_split").cuda()
    assert voc.model.operand_dtype == "f16_split"
    gen = torch.Generator().manual_seed(7)
    x = torch.randint(1, 401, (2, 12), generator=gen).cuda()
    y = torch.randn(2, 128, 40, generator=gen).cuda()
    torch.manual_seed(5)
    mel = tts.synthesise(x, torch.tensor([12, 7]).cuda(), 2, temperature=0.8, y=y, length_scale=1.0, solver="euler", cfg=2.0)["decoder_outputs"]
    audio = voc(mel)
    B, _, T = mel.shape
    assert audio.shape == (B, T * 512) and audio.dtype == torch.float32 and bool(torch.isfinite(audio).all())
    assert float(audio.abs().max()) <= 1.0 and float(audio.std()) > 1e-3
    assert torch.equal(audio, voc(mel.clone())) and torch.equal(audio, voc.model(mel))
    assert voc.model.engine().operand_dtype == "f16_split"
    # the same mel through the default wrapper: the two modes agree to the single rounding's error, and are not the same numbers
    plain = FireflyGANBaseWrapper(path).cuda()(mel)
    diff = float((audio - plain).abs().max() / plain.abs().max())
    assert 0 < diff < 2e-2, diff
