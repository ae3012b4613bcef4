"""FireflyGAN vocoder without a GPU: the float64 restatement against the reference module's fixture, the polyphase map of the
transposed convs, the native module's state_dict layout, the wrapper, the registration and the rejections of unsupported
configurations (tests/golden/ffgan_outputs.npz: tools/make_golden_ffgan.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ffgan_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ffgan_outputs.npz")))


@pytest.fixture(scope="module")
def seeded():
    return R.make_state_dict(R.DEFAULT, R.SEED)


@pytest.fixture(scope="module")
def lib():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_restatement_equals_the_reference_module(gold, seeded, ci):
    B, T = R.CASES[ci]
    out = R.forward(seeded, R.DEFAULT, R.make_mel(B, T, 128, R.MEL_SEED + ci))
    for name in ("audio", "encoder", "pre_tanh"):
        ref = gold[f"{B}x{T}/{name}"]
        assert out[name].shape == ref.shape
        assert R.rel_max(out[name], ref) <= 1e-10, name


@pytest.mark.parametrize("name", list(R.REF_CASES))
def test_restatement_equals_the_reference_modules_at_other_configurations(name):
    """tests/golden/ffgan_config_outputs.npz: the reference's own encoder and head at two non-default configurations."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ffgan_config_outputs.npz"))
    cfg, B, T, mel_seed = R.REF_CASES[name]
    sd = R.make_state_dict(cfg, R.SEED)
    mel = R.make_mel(B, T, cfg["backbone"]["input_channels"], mel_seed)
    out = R.forward(sd, cfg, mel)
    for tensor in ("audio", "encoder", "pre_tanh"):
        ref = gold[f"{name}/{tensor}"]
        assert out[tensor].shape == ref.shape and ref.dtype == np.float64
        assert R.rel_max(out[tensor], ref) <= 1e-10, tensor
    assert out["audio"].shape == (B, T * cfg["head"]["hop_length"])
    for dt in ("f16", "bf16"):      # the recorded e_emul of the GPU gate is the restatement's
        em = R.forward(sd, cfg, mel, dt, dt)
        got = [R.rel_max(em[n], out[n]) for n in ("audio", "encoder", "pre_tanh")]
        want = gold[f"{name}/emul_{dt}"][0]
        assert np.allclose(got, want, rtol=1e-6, atol=0), (dt, got, want)
        assert all(1e-5 < g < 2e-2 for g in got)


def test_emulation_switches_round_and_the_fixture_records_them(gold, seeded):
    """The operand-rounded restatement differs from float64 by what the fixture recorded (case 1x2: the cheapest)."""
    ci, (B, T) = 3, R.CASES[3]
    mel = R.make_mel(B, T, 128, R.MEL_SEED + ci)
    ref = R.forward(seeded, R.DEFAULT, mel)
    for dt in ("f16", "bf16"):
        em = R.forward(seeded, R.DEFAULT, mel, dt, dt)
        got = [R.rel_max(em[n], ref[n]) for n in ("audio", "encoder", "pre_tanh")]
        want = gold[f"{B}x{T}/emul_{dt}"][0]
        assert np.allclose(got, want, rtol=1e-6, atol=0), (dt, got, want)
        assert all(1e-5 < g < 2e-2 for g in got)


@pytest.mark.parametrize("u,k", [(8, 16), (2, 4), (4, 8), (6, 12), (10, 20), (12, 24), (14, 28), (16, 32)])
def test_polyphase_map_equals_conv_transpose(u, k):
    gen = torch.Generator().manual_seed(u)
    x = torch.randn(2, 6, 9, generator=gen, dtype=torch.float64)
    w = torch.randn(6, 5, k, generator=gen, dtype=torch.float64)
    b = torch.randn(5, generator=gen, dtype=torch.float64)
    want = F.conv_transpose1d(x, w, b, stride=u, padding=(k - u) // 2)
    got = R.conv_transpose_polyphase(x, w, b, u)
    assert got.shape == want.shape == (2, 5, 9 * u)
    assert float((got - want).abs().max()) <= 1e-13
    assert int((R.polyphase_weight(w, u) == 0).sum()) == u * 5 * 6      # one third of the packed taps are zero


def test_state_dict_layout_is_the_reference_modules(gold, seeded):
    from stabletts_amd.ffgan import FireflyGANBase
    m = FireflyGANBase()
    sd = m.state_dict()
    names = [str(n) for n in gold["state_names"]]
    shapes = [tuple(int(d) for d in str(s).split(";")) for s in gold["state_shapes"]]
    assert len(names) == 471 and sum(int(np.prod(s)) for s in shapes) == 36511330
    assert list(sd) == names
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert [n for n, _ in R.param_shapes(R.DEFAULT)] == names
    res = m.load_state_dict(seeded, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.state_dict()
    assert all(torch.equal(back[k], seeded[k]) for k in seeded)
    assert not any(p.requires_grad for p in m.parameters())
    # ConvTranspose1d: the weight norm runs over dim 0 = the INPUT channel
    assert tuple(sd["head.ups.0.parametrizations.weight.original0"].shape) == (512, 1, 1)
    assert tuple(sd["head.ups.0.parametrizations.weight.original1"].shape) == (512, 256, 16)


def test_wrapper_loads_a_saved_checkpoint(tmp_path, seeded):
    from stabletts_amd.ffgan import FireflyGANBaseWrapper
    path = str(tmp_path / "generator.ckpt")
    torch.save(seeded, path)
    w = FireflyGANBaseWrapper(path)
    assert not w.model.training
    got = w.model.state_dict()
    assert all(torch.equal(got[k], seeded[k]) for k in seeded)
    bad = dict(seeded)
    bad.pop("head.conv_post.bias")
    torch.save(bad, path)
    with pytest.raises(RuntimeError, match="conv_post.bias"):       # strict, like the reference
        FireflyGANBaseWrapper(path)


def test_install_registers_the_module():
    import stabletts_amd
    saved = {k: sys.modules.pop(k, None) for k in ("vocoders.ffgan.model", "models.flow_matching")}
    try:
        stabletts_amd.install()
        assert "vocoders.ffgan.model" not in sys.modules
        stabletts_amd.install(ffgan=True)
        mod = sys.modules["vocoders.ffgan.model"]
        from stabletts_amd import ffgan
        assert mod is ffgan
        for name in ("config_dict", "ConvNeXtEncoder", "HiFiGANGenerator", "FireflyGANBase", "FireflyGANBaseWrapper"):
            assert hasattr(mod, name), name
        assert stabletts_amd.FireflyGANBase is ffgan.FireflyGANBase
    finally:
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v


def test_config_dict_is_the_reference_default():
    from stabletts_amd.ffgan import config_dict
    assert config_dict == R.DEFAULT


def test_construction_and_argument_rejections():
    from stabletts_amd.ffgan import FireflyGANBase, HiFiGANGenerator
    with pytest.raises(NotImplementedError, match="use_template"):
        HiFiGANGenerator(use_template=True)
    with pytest.raises(AssertionError, match="hop_length"):
        HiFiGANGenerator(hop_length=256, use_template=False)
    with pytest.raises(ValueError, match="operand_dtype"):
        FireflyGANBase(operand_dtype="fp8", config=R.small_config())._create_engine(0)
    cfg = R.small_config()
    cfg["head"]["num_mels"] = 128
    with pytest.raises(ValueError, match="num_mels"):
        FireflyGANBase(config=cfg)
    cfg = R.small_config()
    cfg["head"]["resblock_dilation_sizes"] = [[1, 2], [1]]
    with pytest.raises(ValueError, match="dilations"):
        FireflyGANBase(config=cfg)
    m = FireflyGANBase(config=R.small_config())
    with pytest.raises(ValueError, match="no CPU fallback"):
        m(torch.zeros(1, 64, 4))
    if torch.cuda.is_available():
        m = m.cuda()
        with pytest.raises(ValueError, match="input_channels"):
            m(torch.zeros(1, 65, 4, device="cuda"))
        with pytest.raises(ValueError, match="input_channels"):
            m(torch.zeros(64, 4, device="cuda"))


def _create(lib, cfg):
    from stabletts_amd._lib import StFfganConfig, ffgan_config_fields
    f = ffgan_config_fields(cfg["backbone"], cfg["head"])
    f["operand_dtype"] = cfg.get("operand_dtype", 1)
    h = ctypes.c_void_p()
    rc = lib.st_create_ffgan(ctypes.byref(StFfganConfig(**f)), 0, ctypes.byref(h))
    msg = lib.st_last_error(None).decode()
    if rc == 0:
        lib.st_destroy(h)
    return rc, msg


def _with(section, **over):
    cfg = R.small_config()
    cfg[section].update(over)
    return cfg


UNSUPPORTED = {
    "use_template": (_with("head", use_template=True), "use_template"),
    "k_not_2u": (_with("head", upsample_kernel_sizes=[8, 2]), "2 \\* upsample_rate"),
    "odd_rate": (_with("head", upsample_rates=[3, 2], upsample_kernel_sizes=[6, 4], hop_length=6), "even"),
    "even_resblock_kernel": (_with("head", resblock_kernel_sizes=[4, 5]), "odd"),
    "large_resblock_kernel": (_with("head", resblock_kernel_sizes=[3, 15]), "<= 13"),
    "halo_above_the_patch": (_with("head", resblock_kernel_sizes=[3, 13], resblock_dilation_sizes=[[1, 2], [1, 5]]), "halo"),
    "zero_dilation": (_with("head", resblock_dilation_sizes=[[1, 0], [1, 3]]), "dilations"),
    "head_width_not_16_2n": (_with("head", upsample_initial_channel=96), "16 \\* 2\\^n"),
    "last_level_below_16": (_with("head", upsample_initial_channel=32), "fewer than 16"),
    "even_pre_kernel": (_with("head", pre_conv_kernel_size=6), "pre / post"),
    "large_post_kernel": (_with("head", post_conv_kernel_size=15), "pre / post"),
    "encoder_width": (_with("backbone", dims=[128, 192]) | {"head": {**R.small_config()["head"], "num_mels": 192}}, "multiples of 128"),
    "encoder_width_above_1024": (_with("backbone", dims=[128, 1152]) | {"head": {**R.small_config()["head"], "num_mels": 1152}}, "1024"),
    "encoder_kernel": (_with("backbone", kernel_size=5), "kernel_size == 7"),
    "input_channels": (_with("backbone", input_channels=80), "input_channels"),
    "operand_dtype": ({**R.small_config(), "operand_dtype": 7}, "operand_dtype"),
}


@pytest.mark.parametrize("case", sorted(UNSUPPORTED))
def test_cabi_rejects_unsupported_configurations_without_a_device(lib, case):
    import re
    cfg, pattern = UNSUPPORTED[case]
    rc, msg = _create(lib, cfg)
    assert rc == -1 and re.search(pattern, msg), (rc, msg)      # ST_ERR_INVALID, before any device call


def test_cabi_accepts_supported_configurations(lib):
    """A supported configuration passes the checks: without a device the next failure is the device's (ST_ERR_HIP)."""
    from tests.ffgan_checks import CONFIGS      # every configuration of the GPU tests (test_gpu_ffgan.py, test_gpu_ffgan_configs.py)
    assert set(R.REF_CASES) <= set(CONFIGS) and len(CONFIGS) == 15
    for cfg in (R.DEFAULT, R.small_config(), R.small_config(rates=(2, 2), kernels=(4, 4), rk=(11, 3), rd=((5, 1), (1, 2)), pre=3, post=5),
                *CONFIGS.values()):
        rc, msg = _create(lib, cfg)
        if torch.cuda.is_available():
            assert rc == 0, msg
        else:
            assert rc == -2 and "device" in msg, (rc, msg)
    h = ctypes.c_void_p()
    assert lib.st_create_ffgan(None, 0, ctypes.byref(h)) == -1
    assert lib.st_ffgan_forward(None, None, None, 1, 1, None) == -1
