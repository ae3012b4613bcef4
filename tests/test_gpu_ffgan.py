"""Native FireflyGAN vocoder on a real MI355X against float64: the reference module's fixture at the default configuration
(tests/golden/ffgan_outputs.npz) and the restatement (tests/ffgan_restatement.py) at small configurations.

Accuracy gate, per compared tensor: e_native = max |native - float64| / max |float64| against e_emul, the same figure of the
float64 restatement with weights and conv / linear inputs rounded to the operand dtype where the kernels round:
e_native <= 2 * e_emul (fp32 accumulation order, roundings that flip at ties; a wrong tap, dilation, halo, phase or fold is off by
order 1), and e_emul < 2e-2 (otherwise the input is ill-conditioned and the gate vacuous).  Every pair is printed.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import ffgan_restatement as R
from tests.ffgan_checks import against_restatement, build, gate, run_captured, small_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ffgan_outputs.npz")))


@pytest.fixture(scope="module")
def default_models():
    return {dt: build(R.DEFAULT, dt)[0] for dt in ("f16", "bf16")}


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_default_config_matches_the_reference_fixture(default_models, gold, ci, dt):
    B, T = R.CASES[ci]
    mel = R.make_mel(B, T, 128, R.MEL_SEED + ci)
    got = run_captured(default_models[dt], mel)
    assert got["audio"].shape == (B, T * 512)
    ref = {n: torch.from_numpy(gold[f"{B}x{T}/{n}"]) for n in ("audio", "encoder", "pre_tanh")}
    em = gold[f"{B}x{T}/emul_{dt}"][0]
    gate(f"default {B}x{T} {dt}", got, ref, {"audio": em[0], "encoder": em[1], "pre_tanh": em[2]})


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 31, 33])
def test_frame_tile_edges(T, dt):
    """Level lengths 4 T and 8 T: below one halo (T = 1, 2), and on both sides of 64, 128 and 256 frames (the kernel's tile is 128)."""
    against_restatement("small", dt, 2, T, 300 + T)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["small", "deep16"])
def test_non_default_configs(name, dt):
    against_restatement(name, dt, 2, 21, 41)


def test_items_are_independent_and_runs_repeat_bitwise(default_models):
    m = default_models["f16"]
    mel = R.make_mel(3, 9, 128, 77).cuda()
    a = m(mel)
    b = m(mel)
    assert torch.equal(a, b)
    for i in range(3):
        alone = m(mel[i:i + 1].contiguous())
        assert torch.equal(alone[0], a[i]), i
    ms, _ = small_model("deep16", "bf16")
    mel = R.make_mel(3, 40, 64, 78).cuda()
    a = ms(mel)
    assert torch.equal(a, ms(mel))
    for i in range(3):
        assert torch.equal(ms(mel[i:i + 1].contiguous())[0], a[i]), i


def test_a_batch_that_runs_in_chunks(default_models):
    """B = 10 x T = 1000 needs 10 x 114.7 MB of head workspace: two chunks (9 + 1 utterances) under the 1 GiB bound.  The last item
    of the first chunk and the only item of the second against those utterances alone: the same kernels on the same data, except
    that the encoder's GEMMs may pick another tile shape for another row count (fp32 sums in another order, after which a 16-bit
    rounding can flip): far below the 16-bit operand error itself (2e-3 of max |audio|, profiles/ffgan_parity.txt), which is the
    bound; a wrong chunk offset is off by order 1."""
    m = default_models["f16"]
    mel = R.make_mel(10, 1000, 128, 91).cuda()
    audio = m(mel)
    assert audio.shape == (10, 512000) and bool(torch.isfinite(audio).all())
    for i in (8, 9):
        alone = m(mel[i:i + 1].contiguous())[0]
        err = float((audio[i] - alone).abs().max() / alone.abs().max())
        print(f"ffgan_chunks item {i}: max |in batch - alone| / max = {err:.3e}")
        assert err <= 2e-3, (i, err)


def test_grad_and_device_rules(default_models):
    m = default_models["f16"]
    mel = R.make_mel(1, 4, 128, 5).cuda()
    with torch.enable_grad():       # (GPU tests run under no_grad unless marked grad)
        with pytest.raises(NotImplementedError, match="inference-only"):
            m(mel.clone().requires_grad_(True))
        assert m(mel).shape == (1, 2048)      # parameters and mel without grad: legal in any grad mode
    with torch.no_grad():
        assert m(mel.clone().requires_grad_(True)).shape == (1, 2048)
    with pytest.raises(ValueError, match="no CPU fallback"):
        m(mel.cpu())
    with pytest.raises(ValueError, match="input_channels"):
        m(mel[:, :64].contiguous())


def test_text_to_waveform_through_the_wrapper(tmp_path):
    """The native synthesise chain (text -> mel) feeding the native wrapper, as api.py:75-76 does with its default vocoder."""
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
    mel = tts.synthesise(x, torch.tensor([12, 7]).cuda(), 2, temperature=0.8, y=y, length_scale=1.0, solver="euler", cfg=2.0)["decoder_outputs"]
    audio = voc(mel)
    B, _, T = mel.shape
    assert audio.shape == (B, T * 512) and audio.dtype == torch.float32 and bool(torch.isfinite(audio).all())
    assert float(audio.abs().max()) <= 1.0 and float(audio.std()) > 1e-3
    assert torch.equal(audio, voc(mel.clone()))
    assert torch.equal(audio, voc.model(mel))


def test_entry_points_reject_other_kinds_and_bad_calls(default_models):
    from stabletts_amd import _lib
    from stabletts_amd._lib import NativeError
    m = default_models["f16"]
    eng = m.engine()
    lib = eng.lib
    mel = torch.zeros(1, 128, 4, device="cuda")
    audio = torch.zeros(1, 2048, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(NativeError, match="not a vocoder"):                     # a Vocos entry point on an ffgan handle
        eng.vocos_forward(mel, audio, s)
    with pytest.raises(NativeError, match="vocoder handles re-pack through st_finalize"):
        eng.repack(s)
    voc = _lib.Engine(0, 0, 0, 0, 0, 0, 0, "f16", 0, vocoder=dict(input_channels=128, dim=512, intermediate_dim=1536, num_layers=8, n_fft=2048, hop_length=512))
    with pytest.raises(NativeError, match="not a FireflyGAN vocoder"):          # ... and the ffgan entry point on a Vocos handle
        voc.ffgan_forward(mel, audio, s)
    voc.close()
    h = eng.handle
    assert lib.st_ffgan_forward(h, None, audio.data_ptr(), 1, 4, ctypes.c_void_p(s)) == -1 and b"null" in lib.st_last_error(h)
    assert lib.st_ffgan_forward(h, mel.data_ptr(), audio.data_ptr(), 0, 4, ctypes.c_void_p(s)) == -1
    assert lib.st_ffgan_forward(h, mel.data_ptr(), audio.data_ptr(), 1, (1 << 20) + 1, ctypes.c_void_p(s)) == -1
    assert b"T too large" in lib.st_last_error(h)
    fresh = _lib.Engine(0, 0, 0, 0, 0, 0, 0, "f16", 0, ffgan=m._fields)
    with pytest.raises(NativeError, match="st_finalize"):                       # forward before the parameters are loaded
        fresh.ffgan_forward(mel, audio, s)
    with pytest.raises(NativeError, match="shape mismatch"):
        fresh.load_state_dict({"head.ups.0.parametrizations.weight.original0": torch.zeros(256, 1, 1)})
    with pytest.raises(NativeError, match="unexpected parameter name"):
        fresh.load_state_dict({"head.noise_convs.0.weight": torch.zeros(1)})
    fresh.close()
    assert m(mel).shape == (1, 2048)                                            # the handle still works after the rejected calls
