"""CPU checks of the native multi-resolution discriminator: the torch restatement (tests/mrd_restatement.py) against the float64
feature maps and gradients of the REAL reference module (tests/golden/mrd_grads.npz, tools/make_golden_mrd.py), the module /
install rules that need no device, and the new C entry points' symbols and host-side argument checks."""
import ctypes
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import mrd_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-10         # relative L2 per tensor: both sides are float64 and differ only in summation order (and FFT against DFT)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mrd_grads.npz")))


@pytest.mark.parametrize("case", sorted(R.LINEAR_CASES))
def test_restatement_reproduces_the_linear_cases(gold, case):
    W, B, T, wseed, aseed = R.LINEAR_CASES[case]
    sd = R.to_torch(R.make_dr_state_dict(wseed), requires_grad=True)
    x = torch.from_numpy(R.make_audio(B, T, aseed)).double().requires_grad_(True)
    out = R.forward(sd, x, W, 1.0)
    loss = R.linear_loss(out.fmaps, wseed)
    loss.backward()
    l64 = float(gold[case + "/loss64"].reshape(-1)[0])
    assert abs(float(loss.detach()) - l64) <= BAR * abs(l64)
    assert len(out.fmaps) == 21 and [",".join(map(str, f.shape)) for f in out.fmaps] == gold[case + "/fmap_shapes"].tolist()
    worst = 0.0
    for i, f in enumerate(out.fmaps):
        worst = max(worst, R.rel_l2(R.stored(1000 + i, f.detach().numpy(), wseed), gold[f"{case}/fmap/{i}"]))
    names = gold[case + "/names"].tolist()
    assert names == list(sd)
    for i, n in enumerate(names):
        worst = max(worst, R.rel_l2(R.stored(i, sd[n].grad.numpy(), wseed), gold[f"{case}/grad/{n}"]))
    worst = max(worst, R.rel_l2(x.grad.numpy(), gold[case + "/dx64"]))
    print(f"{case}: worst relative L2 to the real module {worst:.2e} (bar {BAR:.0e})")
    assert worst <= BAR


def test_restatement_reproduces_the_train_step(gold):
    seed, B, T = int(gold["train_step/seed"].reshape(-1)[0]), R.TRAIN_STEP["B"], R.TRAIN_STEP["T"]
    sd = R.to_torch(R.make_mrd_state_dict(seed), requires_grad=True)
    y = torch.from_numpy(R.make_audio(B, T, seed + 1)).double()
    yh = torch.from_numpy(R.make_audio(B, T, seed + 2)).double().requires_grad_(True)
    outs = R.mrd_forward(sd, y, yh)
    loss, parts, _ = R.gan_losses(outs, B)
    loss.backward()
    got = np.array([float(parts[k].detach()) for k in ("disc", "feat", "gen")])
    assert np.all(np.abs(got - gold["train_step/losses64"]) <= BAR * np.abs(gold["train_step/losses64"]))
    assert list(sd) == gold["train_step/names"].tolist()
    worst = 0.0
    for i, n in enumerate(sd):
        worst = max(worst, R.rel_l2(R.stored(i, sd[n].grad.numpy(), seed), gold[f"train_step/grad/{n}"]))
    worst = max(worst, R.rel_l2(yh.grad.numpy(), gold["train_step/dyhat64"]))
    for k, o in enumerate(outs):
        assert len(o.fmaps) == 21
        for i, f in enumerate(o.fmaps):
            worst = max(worst, R.rel_l2(R.stored(2000 + 100 * k + i, f.detach().numpy(), seed), gold[f"train_step/fmap/{k}/{i}"]))
        worst = max(worst, R.rel_l2(o.fmaps[-1].detach().numpy(), gold[f"train_step/logits/{k}"]))
    print(f"train_step: worst relative L2 to the real module {worst:.2e} (bar {BAR:.0e})")
    assert worst <= BAR


def test_supplied_signs_are_the_same_function_when_they_are_its_own():
    """A self-check of the test infrastructure (tests/mrd_restatement.py alone, no native code): the sign-supplied path every GPU
    gradient comparison leans on is the same function at the restatement's own signs, and another one at a flipped sign."""
    W, B, T, seed = 64, 2, 97, 31
    sd_np, x_np = R.make_dr_state_dict(seed), R.make_audio(B, T, seed + 1)
    res = []
    for supplied in (False, True):
        sd = R.to_torch(sd_np, requires_grad=True)
        x = torch.from_numpy(x_np).double().requires_grad_(True)
        signs = R.forward(R.to_torch(sd_np), x.detach(), W).signs if supplied else None
        out = R.forward(sd, x, W, signs=signs)
        R.linear_loss(out.fmaps, seed).backward()
        res.append(({n: t.grad.clone() for n, t in sd.items()}, x.grad.clone(), out))
    (ga, da, oa), (gb, db, _) = res
    assert torch.equal(da, db) and all(torch.equal(ga[n], gb[n]) for n in ga)
    flipped = [[s.clone() for s in band] for band in oa.signs]
    flipped[2][0].view(-1)[0] ^= True                     # a layer-0 sign, which no returned map shows
    other = R.forward(R.to_torch(sd_np), torch.from_numpy(x_np).double(), W, signs=flipped)
    assert not torch.equal(other.fmaps[-1], oa.fmaps[-1].detach())


def test_module_tree_and_state_dict_are_the_reference_modules(gold):
    """Key names, their order and the shapes of DiscriminatorR and MultiResolutionDiscriminator equal what the REAL modules gave the
    generator; a seeded state dict loads with strict=True; the constructors' signatures are the reference's; non-native
    configurations raise at construction; no CPU fallback."""
    from stabletts_amd.discriminator import DiscriminatorR, MultiResolutionDiscriminator
    d = DiscriminatorR(32)
    sd = d.state_dict()
    assert list(sd) == gold["linear_w32/state_names"].tolist() and len(sd) == 79 and list(sd)[0] == "spec_fn.window"
    assert [",".join(map(str, v.shape)) for v in sd.values()] == gold["linear_w32/state_shapes"].tolist()
    assert [n for n, _ in d.named_parameters()] == gold["linear_w32/names"].tolist()
    assert [",".join(map(str, q.shape)) for q in d.parameters()] == gold["linear_w32/shapes"].tolist()
    assert torch.equal(sd["spec_fn.window"], torch.hann_window(32))
    assert d.bands == [(0, 1), (1, 4), (4, 8), (8, 12), (12, 17)] and d.window_length == 32 and d.hop_factor == 0.25
    m = MultiResolutionDiscriminator()
    sd = m.state_dict()
    assert list(sd) == gold["train_step/state_names"].tolist()          # the real module's: 234 parameters + 3 spec_fn.window buffers
    assert [",".join(map(str, v.shape)) for v in sd.values()] == gold["train_step/state_shapes"].tolist()
    assert [n for n, _ in m.named_parameters()] == gold["train_step/names"].tolist()
    assert [",".join(map(str, q.shape)) for q in m.parameters()] == gold["train_step/shapes"].tolist()
    full = {k: torch.from_numpy(v) for k, v in R.with_windows(R.make_mrd_state_dict(5)).items()}
    m.load_state_dict(full, strict=True)
    with pytest.raises(RuntimeError, match="spec_fn.window"):          # as the reference: a checkpoint without the windows is not strict
        m.load_state_dict({k: v for k, v in full.items() if not k.endswith("window")}, strict=True)
    assert [q.window_length for q in m.discriminators] == [2048, 1024, 512]
    assert len(sd) == 237 and len(list(m.parameters())) == 234
    assert sum(q.numel() for q in m.parameters()) == 1413990 and all(q.requires_grad for q in m.parameters())
    assert "discriminators.1.band_convs.3.2.parametrizations.weight.original1" in sd and "discriminators.2.conv_post.bias" in sd
    assert "discriminators.0.spec_fn.window" in sd and sd["discriminators.0.spec_fn.window"].shape == (2048,)
    # the reference's signatures (vocoders/vocos/models/discriminator.py:79-82,113-119)
    sig = inspect.signature(DiscriminatorR.__init__).parameters
    assert list(sig) == ["self", "window_length", "channels", "hop_factor", "bands"]
    assert (sig["channels"].default, sig["hop_factor"].default) == (32, 0.25)
    assert sig["bands"].default == ((0.0, 0.1), (0.1, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0))
    sig = inspect.signature(MultiResolutionDiscriminator.__init__).parameters
    assert list(sig) == ["self", "fft_sizes"] and sig["fft_sizes"].default == (2048, 1024, 512)
    assert list(inspect.signature(m.forward).parameters) == ["y", "y_hat"]
    assert list(inspect.signature(d.forward).parameters) == ["x"]
    # what is not built natively raises at construction, naming the limits
    for bad in (dict(window_length=16), dict(window_length=4096), dict(window_length=48), dict(window_length=64, channels=16),
                dict(window_length=64, hop_factor=0.5), dict(window_length=64, bands=((0.0, 0.5), (0.5, 1.0))),
                dict(window_length=64, bands=((0.0, 0.1), (0.1, 0.1), (0.1, 0.5), (0.5, 0.75), (0.75, 1.0))),
                dict(window_length=64, bands=((0.0, 0.1), (0.1, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.5)))):
        with pytest.raises(NotImplementedError, match=r"power of two in \[32, 2048\], channels=32, hop_factor=0.25"):
            DiscriminatorR(**bad)
    with pytest.raises(NotImplementedError):
        MultiResolutionDiscriminator(fft_sizes=(2048, 16))
    ok = DiscriminatorR(64, bands=((0.0, 0.3), (0.2, 0.5), (0.5, 0.6), (0.6, 0.9), (0.9, 1.0)))      # overlapping, uneven: built
    assert ok.bands == [(0, 9), (6, 16), (16, 19), (19, 29), (29, 33)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d(torch.zeros(1, 1, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 4096), torch.zeros(1, 1, 4096))


def test_install_rebinds_the_two_resolution_names_in_the_users_module():
    import stabletts_amd
    from stabletts_amd import discriminator as nd
    assert stabletts_amd.MultiResolutionDiscriminator is nd.MultiResolutionDiscriminator
    names = ["vocoders", "vocoders.vocos", "vocoders.vocos.models", "vocoders.vocos.models.discriminator", "models.flow_matching"]
    saved = {k: sys.modules.pop(k, None) for k in names}
    try:
        stub = types.ModuleType("vocoders.vocos.models.discriminator")
        stub.MultiPeriodDiscriminator, stub.DiscriminatorP = object(), object()
        stub.MultiResolutionDiscriminator, stub.DiscriminatorR, stub.weight_norm = object(), object(), object()
        others = {k: getattr(stub, k) for k in ("MultiPeriodDiscriminator", "DiscriminatorP", "weight_norm")}
        for k in names[:3]:
            sys.modules[k] = types.ModuleType(k)
            sys.modules[k].__path__ = []
        sys.modules[names[3]] = stub
        stabletts_amd.install(resolution_discriminator="train")
        assert stub.MultiResolutionDiscriminator is nd.MultiResolutionDiscriminator and stub.DiscriminatorR is nd.DiscriminatorR
        assert all(getattr(stub, k) is v for k, v in others.items())
        stabletts_amd.install(discriminator="train", resolution_discriminator="train")       # both: all four names
        assert stub.MultiPeriodDiscriminator is nd.MultiPeriodDiscriminator and stub.DiscriminatorR is nd.DiscriminatorR
        for bad in (True, "eval", 1):
            with pytest.raises(ValueError, match='"train"'):
                stabletts_amd.install(resolution_discriminator=bad)
        del sys.modules[names[3]]
        with pytest.raises(ImportError, match="vocoders.vocos.models.discriminator"):
            stabletts_amd.install(resolution_discriminator="train")
    finally:
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v


def test_abi_symbols_and_host_side_argument_checks():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    lib = _lib.load()
    for name in ("st_create_resolution_discriminator", "st_resolution_disc_fmap_shape", "st_resolution_disc_forward",
                 "st_resolution_disc_train_forward", "st_resolution_disc_train_backward", "st_resolution_disc_wgrad_planes"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    assert ctypes.sizeof(_lib.StResolutionDiscConfig) == 48

    def cfg(W=64, slope=0.1, **over):
        d = dict(window_length=W, lrelu_slope=slope)
        for c, (lo, hi) in enumerate(R.band_ranges(W)):
            d[f"band_lo{c}"], d[f"band_hi{c}"] = lo, hi
        d.update(over)
        return _lib.StResolutionDiscConfig(**d)

    h = ctypes.c_void_p()
    ok = cfg()
    assert lib.st_create_resolution_discriminator(None, 0, ctypes.byref(h)) == _lib.ST_ERR_INVALID
    assert lib.st_last_error(None).decode() == "null argument"
    assert lib.st_create_resolution_discriminator(ctypes.byref(ok), 0, None) == _lib.ST_ERR_INVALID
    for bad in (cfg(slope=0.0), cfg(slope=-0.1), cfg(slope=float("nan")), cfg(band_lo0=-1), cfg(band_hi4=34)):
        assert lib.st_create_resolution_discriminator(ctypes.byref(bad), 0, ctypes.byref(h)) == _lib.ST_ERR_INVALID
        assert not h.value
    for bad, msg in ((cfg(W=16), "power of two"), (cfg(W=4096), "power of two"), (cfg(W=96), "power of two"),
                     (cfg(band_hi1=2), "at least one bin"), (cfg(band_lo3=24, band_hi3=24), "at least one bin")):
        assert lib.st_create_resolution_discriminator(ctypes.byref(bad), 0, ctypes.byref(h)) == _lib.ST_ERR_UNSUPPORTED
        assert msg in lib.st_last_error(None).decode() and not h.value
    if not torch.cuda.is_available():
        assert lib.st_create_resolution_discriminator(ctypes.byref(ok), 0, ctypes.byref(h)) == _lib.ST_ERR_HIP
        assert lib.st_last_error(None).decode() == "no such HIP device"
    ptrs = (ctypes.c_void_p * 21)()
    c, f, w = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.st_resolution_disc_fmap_shape(None, 64, 0, ctypes.byref(c), ctypes.byref(f), ctypes.byref(w)) == _lib.ST_ERR_INVALID
    assert lib.st_resolution_disc_wgrad_planes(None, 1, 64, 0, 0) == _lib.ST_ERR_INVALID
    assert lib.st_resolution_disc_forward(None, None, ptrs, 1, 64, None) == _lib.ST_ERR_INVALID
    assert lib.st_resolution_disc_train_forward(None, None, ptrs, 0, 0, None) == _lib.ST_ERR_INVALID
    assert lib.st_resolution_disc_train_backward(None, ptrs, None, None, 1, 64, None) == _lib.ST_ERR_INVALID
