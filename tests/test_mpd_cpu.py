"""CPU checks of the native multi-period discriminator: the torch restatement (tests/mpd_restatement.py) against the float64
feature maps and gradients of the REAL reference module (tests/golden/mpd_grads.npz, tools/make_golden_mpd.py), the weight-norm
backward formula, the sign-supplied path, the module / install rules that need no device, and the new C entry points' symbols
and host-side argument checks."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import mpd_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-10         # relative L2 per tensor: both sides are float64 and differ only in summation order


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mpd_grads.npz")))


@pytest.mark.parametrize("case", sorted(R.LINEAR_CASES))
def test_restatement_reproduces_the_linear_cases(gold, case):
    p, B, T, wseed, aseed = R.LINEAR_CASES[case]
    sd = R.to_torch(R.make_dp_state_dict(wseed), requires_grad=True)
    x = torch.from_numpy(R.make_audio(B, T, aseed)).double().requires_grad_(True)
    out = R.forward(sd, x, p, 1.0)
    loss = R.linear_loss(out.fmaps, wseed)
    loss.backward()
    l64 = float(gold[case + "/loss64"].reshape(-1)[0])
    assert abs(float(loss.detach()) - l64) <= BAR * abs(l64)
    assert [",".join(map(str, f.shape)) for f in out.fmaps] == gold[case + "/fmap_shapes"].tolist()
    worst = 0.0
    for i, f in enumerate(out.fmaps):
        worst = max(worst, R.rel_l2(R.stored_elements(1000 + i, f.detach().numpy(), wseed), gold[f"{case}/fmap/{i}"]))
    for i, n in enumerate(gold[case + "/names"].tolist()):
        worst = max(worst, R.rel_l2(R.stored_elements(i, sd[n].grad.numpy(), wseed), gold[f"{case}/grad/{n}"]))
    worst = max(worst, R.rel_l2(x.grad.numpy(), gold[case + "/dx64"]))
    print(f"{case}: worst relative L2 to the real module {worst:.2e} (bar {BAR:.0e})")
    assert worst <= BAR


def _train_step_inputs(gold, B=None, T=None):
    ts, seed = R.TRAIN_STEP, int(gold["train_step/seed"].reshape(-1)[0])
    B, T = B or ts["B"], T or ts["T"]
    return seed, R.make_mpd_state_dict(seed), R.make_audio(B, T, seed + 1), R.make_audio(B, T, seed + 2)


def test_restatement_reproduces_the_train_step(gold):
    seed, sd_np, y_np, yh_np = _train_step_inputs(gold)
    sd = R.to_torch(sd_np, requires_grad=True)
    y, yh = torch.from_numpy(y_np).double(), torch.from_numpy(yh_np).double().requires_grad_(True)
    outs = R.mpd_forward(sd, y, yh, R.TRAIN_STEP["slope"])
    loss, parts, _ = R.gan_losses(outs, y.shape[0])
    loss.backward()
    got = np.array([float(parts[k].detach()) for k in ("disc", "feat", "gen")])
    assert np.all(np.abs(got - gold["train_step/losses64"]) <= BAR * np.abs(gold["train_step/losses64"]))
    assert list(sd) == gold["train_step/names"].tolist()
    worst = 0.0
    for i, n in enumerate(sd):
        worst = max(worst, R.rel_l2(R.stored_elements(i, sd[n].grad.numpy(), seed), gold[f"train_step/grad/{n}"]))
    worst = max(worst, R.rel_l2(yh.grad.numpy(), gold["train_step/dyhat64"]))
    for k, o in enumerate(outs):
        for i, f in enumerate(o.fmaps):
            worst = max(worst, R.rel_l2(R.stored_elements(2000 + 10 * k + i, f.detach().numpy(), seed), gold[f"train_step/fmap/{k}/{i}"]))
        worst = max(worst, R.rel_l2(o.fmaps[-1].detach().numpy().reshape(2 * y.shape[0], -1), gold[f"train_step/logits/{k}"]))
        assert o.margin0 > 64 * 2.0 ** -24          # layer 0's pre-activations stand clear of fp32 rounding: its signs are safe to share
    print(f"train_step: worst relative L2 to the real module {worst:.2e} (bar {BAR:.0e})")
    assert worst <= BAR


def test_weight_norm_backward_formula_is_autograd_of_the_parametrisation():
    from torch.nn.utils.parametrizations import weight_norm
    torch.manual_seed(3)
    conv = weight_norm(torch.nn.Conv2d(6, 4, (5, 1))).double()
    g, v = conv.parametrizations.weight.original0, conv.parametrizations.weight.original1
    with torch.no_grad():
        g.mul_(torch.rand_like(g) + 0.5)
    dw = torch.randn_like(v)
    (conv.weight * dw).sum().backward()
    dg, dv = R.weight_norm_backward(dw, v.detach(), g.detach())
    assert torch.equal(R.weight_norm_w(v, g), conv.weight) or R.rel_l2(R.weight_norm_w(v, g).detach(), conv.weight.detach()) <= BAR
    assert R.rel_l2(dg, g.grad) <= BAR and R.rel_l2(dv, v.grad) <= BAR
    assert float(g.grad.abs().min()) > 0 and float(v.grad.abs().max()) > 0


def test_supplied_signs_are_the_same_function_when_they_are_its_own(gold):
    seed, sd_np, y_np, yh_np = _train_step_inputs(gold, B=1, T=97)
    res = []
    for supplied in (False, True):
        sd = R.to_torch(sd_np, requires_grad=True)
        y, yh = torch.from_numpy(y_np).double(), torch.from_numpy(yh_np).double().requires_grad_(True)
        signs = l1 = None
        if supplied:
            with torch.no_grad():
                ref = R.mpd_forward(R.to_torch(sd_np), y, yh.detach(), 0.1)
                signs, l1 = [o.signs for o in ref], R.gan_losses(ref, 1)[2]
        outs = R.mpd_forward(sd, y, yh, 0.1, signs=signs)
        loss, _, _ = R.gan_losses(outs, 1, l1)
        loss.backward()
        res.append((float(loss.detach()), {n: t.grad.clone() for n, t in sd.items()}, yh.grad.clone()))
    (la, ga, da), (lb, gb, db) = res
    assert la == lb and torch.equal(da, db) and all(torch.equal(ga[n], gb[n]) for n in ga)
    # and a flipped sign is another function: the comparison would notice a kernel that picks its own branches
    sd = R.to_torch(sd_np)
    ref = R.forward(sd, torch.from_numpy(y_np).double(), 2, 0.1, prefix="discriminators.0.")
    flipped = [s.clone() for s in ref.signs]
    flipped[2].view(-1)[0] ^= True
    other = R.forward(sd, torch.from_numpy(y_np).double(), 2, 0.1, signs=flipped, prefix="discriminators.0.")
    assert not torch.equal(other.fmaps[-1], ref.fmaps[-1])


def test_module_tree_and_state_dict_are_the_reference_modules(gold):
    """Key names, their order and the shapes of DiscriminatorP and MultiPeriodDiscriminator equal what the REAL modules gave the
    generator; a seeded state dict loads with strict=True; non-native configurations raise at construction; no CPU fallback."""
    import inspect
    from stabletts_amd.discriminator import DiscriminatorP, MultiPeriodDiscriminator
    d = DiscriminatorP(3)
    sd = d.state_dict()
    assert list(sd) == gold["linear_p3/names"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == gold["linear_p3/shapes"].tolist()
    m = MultiPeriodDiscriminator()
    sd = m.state_dict()
    assert list(sd) == gold["train_step/names"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == gold["train_step/shapes"].tolist()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.make_mpd_state_dict(5).items()}, strict=True)
    assert [q.period for q in m.discriminators] == [2, 3, 5, 7, 11] and all(q.lrelu_slope == 0.1 for q in m.discriminators)
    assert sum(q.numel() for q in m.parameters()) == 41105770 and all(q.requires_grad for q in m.parameters())
    assert list(inspect.signature(DiscriminatorP.__init__).parameters) == ["self", "period", "in_channels", "kernel_size", "stride", "lrelu_slope"]
    assert list(inspect.signature(m.forward).parameters) == ["y", "y_hat"]
    for bad in (dict(in_channels=2), dict(kernel_size=3), dict(stride=2)):
        with pytest.raises(NotImplementedError, match="in_channels=1, kernel_size=5, stride=3"):
            DiscriminatorP(2, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d(torch.zeros(1, 1, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 64), torch.zeros(1, 1, 64))


def test_install_rebinds_the_two_names_in_the_users_module():
    import stabletts_amd
    from stabletts_amd import discriminator as nd
    names = ["vocoders", "vocoders.vocos", "vocoders.vocos.models", "vocoders.vocos.models.discriminator", "models.flow_matching"]
    saved = {k: sys.modules.pop(k, None) for k in names}
    try:
        stub = types.ModuleType("vocoders.vocos.models.discriminator")
        stub.MultiPeriodDiscriminator, stub.DiscriminatorP = object(), object()
        stub.MultiResolutionDiscriminator, stub.DiscriminatorR, stub.weight_norm = object(), object(), object()
        others = {k: getattr(stub, k) for k in ("MultiResolutionDiscriminator", "DiscriminatorR", "weight_norm")}
        for k in names[:3]:
            sys.modules[k] = types.ModuleType(k)
            sys.modules[k].__path__ = []
        sys.modules[names[3]] = stub
        stabletts_amd.install(discriminator="train")
        assert stub.MultiPeriodDiscriminator is nd.MultiPeriodDiscriminator and stub.DiscriminatorP is nd.DiscriminatorP
        assert all(getattr(stub, k) is v for k, v in others.items())
        with pytest.raises(ValueError, match='"train"'):
            stabletts_amd.install(discriminator=True)
        del sys.modules[names[3]]
        with pytest.raises(ImportError, match="vocoders.vocos.models.discriminator"):
            stabletts_amd.install(discriminator="train")
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
    for name in ("st_create_period_discriminator", "st_period_disc_fmap_shape", "st_period_disc_forward", "st_period_disc_train_forward",
                 "st_period_disc_train_backward"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    h = ctypes.c_void_p()
    ok = _lib.StPeriodDiscConfig(period=3, lrelu_slope=0.1)
    assert lib.st_create_period_discriminator(None, 0, ctypes.byref(h)) == _lib.ST_ERR_INVALID
    assert lib.st_last_error(None).decode() == "null argument"
    assert lib.st_create_period_discriminator(ctypes.byref(ok), 0, None) == _lib.ST_ERR_INVALID
    for bad in (dict(period=0), dict(period=-2), dict(lrelu_slope=0.0), dict(lrelu_slope=-0.1), dict(lrelu_slope=float("nan"))):
        cfg = _lib.StPeriodDiscConfig(**{**dict(period=3, lrelu_slope=0.1), **bad})
        assert lib.st_create_period_discriminator(ctypes.byref(cfg), 0, ctypes.byref(h)) == _lib.ST_ERR_INVALID, bad
        assert not h.value
    if not torch.cuda.is_available():
        assert lib.st_create_period_discriminator(ctypes.byref(ok), 0, ctypes.byref(h)) == _lib.ST_ERR_HIP
        assert lib.st_last_error(None).decode() == "no such HIP device"
    ptrs = (ctypes.c_void_p * 5)()
    c, r = ctypes.c_int64(), ctypes.c_int64()
    assert lib.st_period_disc_fmap_shape(None, 64, 0, ctypes.byref(c), ctypes.byref(r)) == _lib.ST_ERR_INVALID
    assert lib.st_period_disc_forward(None, None, ptrs, 1, 64, None) == _lib.ST_ERR_INVALID
    assert lib.st_period_disc_train_forward(None, None, ptrs, 0, 0, None) == _lib.ST_ERR_INVALID
    assert lib.st_period_disc_train_backward(None, ptrs, None, None, 1, 64, None) == _lib.ST_ERR_INVALID
