"""CPU checks of the fused GAN losses (stabletts_amd/gan_loss.py): the fallback path against the plain expressions in values,
gradients and return structures, install(gan_losses=True) on stub modules, and the new C entry points' symbols and host-side
argument checks (no device is touched)."""
import ctypes
import sys
import types

import pytest
import torch


def _maps(seed, requires_grad):
    g = torch.Generator().manual_seed(seed)
    shapes = [[(2, 3, 5), (2, 1, 7)], [(2, 4), (2, 2, 2, 3), (2, 1)]]
    return [[torch.randn(s, generator=g).requires_grad_(requires_grad) for s in d] for d in shapes]


def _plain_feature(fmap_r, fmap_g):
    return 2 * sum(torch.mean(torch.abs(rl - gl)) for dr, dg in zip(fmap_r, fmap_g) for rl, gl in zip(dr, dg))


def test_feature_loss_fallback_is_the_plain_expression():
    from stabletts_amd import gan_loss as G
    r, g = _maps(1, True), _maps(2, True)
    r2, g2 = [[t.detach().clone().requires_grad_(True) for t in d] for d in r], [[t.detach().clone().requires_grad_(True) for t in d] for d in g]
    loss, want = G.feature_loss(r, g), _plain_feature(r2, g2)
    assert isinstance(loss, torch.Tensor) and loss.dim() == 0 and torch.equal(loss.detach(), want.detach())
    (loss * 0.37).backward()
    (want * 0.37).backward()
    for a, b in zip([t for d in r + g for t in d], [t for d in r2 + g2 for t in d]):
        assert a.grad is not None and torch.equal(a.grad, b.grad)            # the real maps are not detached
    # float64 inputs take the fallback as well, and keep their dtype
    assert G.feature_loss([[t.detach().double() for t in d] for d in r], [[t.detach().double() for t in d] for d in g]).dtype == torch.float64
    assert G.feature_loss([], []) == 0


def test_discriminator_and_generator_loss_fallback_and_return_structures():
    from stabletts_amd import gan_loss as G
    g = torch.Generator().manual_seed(3)
    shapes = [(2, 1), (2, 7), (3, 1, 5, 9)]
    dr = [torch.randn(s, generator=g).requires_grad_(True) for s in shapes]
    dg = [torch.randn(s, generator=g).requires_grad_(True) for s in shapes]
    out = G.discriminator_loss(dr, dg)
    assert isinstance(out, tuple) and len(out) == 3
    loss, r_losses, g_losses = out
    want_r, want_g = [torch.mean((1 - t.detach()) ** 2) for t in dr], [torch.mean(t.detach() ** 2) for t in dg]
    assert loss.dim() == 0 and torch.equal(loss.detach(), sum(a + b for a, b in zip(want_r, want_g)).detach())
    assert all(type(v) is float for v in r_losses + g_losses) and len(r_losses) == len(g_losses) == 3
    assert r_losses == [float(v) for v in want_r] and g_losses == [float(v) for v in want_g]
    loss.backward()
    for t in dr:
        assert torch.allclose(t.grad, 2 * (t.detach() - 1) / t.numel(), rtol=1e-6, atol=0)
    for t in dg:
        assert torch.allclose(t.grad, 2 * t.detach() / t.numel(), rtol=1e-6, atol=0)

    x = [t.detach().clone().requires_grad_(True) for t in dg]
    out = G.generator_loss(x)
    assert isinstance(out, tuple) and len(out) == 2
    loss, gen_losses = out
    want = [torch.mean((1 - t.detach()) ** 2) for t in x]
    assert loss.dim() == 0 and torch.equal(loss.detach(), sum(want))
    assert len(gen_losses) == 3 and all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in gen_losses)
    assert all(torch.equal(a.detach(), b) for a, b in zip(gen_losses, want))
    loss.backward()
    for t in x:
        assert torch.allclose(t.grad, 2 * (t.detach() - 1) / t.numel(), rtol=1e-6, atol=0)


def test_halves_of_one_base_are_recognised_only_where_both_sides_carry_gradient():
    from stabletts_amd.gan_loss import _halves_base
    leaf = torch.randn(4, 3, 5, requires_grad=True)
    f = leaf * 1
    assert _halves_base(f[:2], f[2:]) is f and _halves_base(f[:1], f[1:]) is f
    lg = torch.flatten(f, 1, -1)
    assert _halves_base(lg[:2], lg[2:]) is f                              # views of views reach the same base
    assert _halves_base(f[2:], f[:2]) is None                             # the wrong way round
    assert _halves_base(f[:2], f[3:]) is None and _halves_base(f[:1], f[2:]) is None       # do not tile the base
    assert _halves_base(f[:2].detach(), f[2:]) is None and _halves_base(f[:2], f[2:].detach()) is None
    assert _halves_base(f[:, :1], f[:, 1:]) is None                       # not contiguous
    assert _halves_base(f[:2].clone(), f[2:].clone()) is None             # tensors of their own
    ft = leaf.transpose(0, 1)
    assert _halves_base(ft[:1], ft[1:]) is None                           # the base's own layout is leaf's, not the views'
    nog = torch.randn(4, 3)
    assert _halves_base(nog[:2], nog[2:]) is None


def test_install_rebinds_the_three_names_in_the_users_module():
    import stabletts_amd
    from stabletts_amd import gan_loss as G
    names = ["vocoders", "vocoders.vocos", "vocoders.vocos.models", "vocoders.vocos.models.loss", "models.flow_matching"]
    saved = {k: sys.modules.pop(k, None) for k in names}
    try:
        stub = types.ModuleType("vocoders.vocos.models.loss")
        stub.feature_loss, stub.discriminator_loss, stub.generator_loss = object(), object(), object()
        stub.MultiScaleMelSpectrogramLoss, stub.SingleScaleMelSpectrogramLoss = object(), object()
        others = {k: getattr(stub, k) for k in ("MultiScaleMelSpectrogramLoss", "SingleScaleMelSpectrogramLoss")}
        for k in names[:3]:
            sys.modules[k] = types.ModuleType(k)
            sys.modules[k].__path__ = []
        sys.modules[names[3]] = stub
        stabletts_amd.install()                                           # the default leaves the module alone
        assert not any(getattr(stub, k) is getattr(G, k) for k in G.__all__)
        stabletts_amd.install(gan_losses=True)
        assert all(getattr(stub, k) is getattr(G, k) for k in ("feature_loss", "discriminator_loss", "generator_loss"))
        assert all(getattr(stub, k) is v for k, v in others.items())
        del sys.modules[names[3]]
        with pytest.raises(ImportError, match="vocoders.vocos.models.loss"):
            stabletts_amd.install(gan_losses=True)
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
    for name in ("st_gan_loss_scratch_bytes", "st_gan_loss_chunk", "st_gan_loss_max_pairs", "st_feature_loss_forward",
                 "st_feature_loss_backward", "st_lsgan_loss_forward", "st_lsgan_loss_backward"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    C, P = lib.st_gan_loss_chunk(), lib.st_gan_loss_max_pairs()
    assert C >= 1024 and C % 1024 == 0 and P >= 2 and P * 48 <= 3072          # the tables travel as kernel arguments
    INV = _lib.ST_ERR_INVALID
    i64s = lambda *v: (ctypes.c_int64 * len(v))(*v)       # noqa: E731
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)      # noqa: E731

    # scratch: one fp64 partial per chunk and one fp64 mean per entry
    assert lib.st_gan_loss_scratch_bytes(i64s(1), 1) == 16
    assert lib.st_gan_loss_scratch_bytes(i64s(C, C + 1, 3 * C + 5), 3) == 8 * (1 + 2 + 4 + 3)
    assert lib.st_gan_loss_scratch_bytes(None, 0) == 0
    assert lib.st_gan_loss_scratch_bytes(None, 1) == INV and lib.st_gan_loss_scratch_bytes(i64s(4), -1) == INV
    assert lib.st_gan_loss_scratch_bytes(i64s(4, 0), 2) == INV and lib.st_gan_loss_scratch_bytes(i64s(-4), 1) == INV
    assert lib.st_last_error(None).decode() == "every element count must be >= 1"

    # fake but well-formed device addresses: every call below must return before anything is launched
    a, b, out, scr, g = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    n1 = i64s(10)
    ok = dict(fwd=(ptrs(a), ptrs(b), n1, 1, out, scr, 16, None), bwd=(ptrs(a), ptrs(b), n1, 1, g, ptrs(a), ptrs(b), None),
              lfwd=(ptrs(a), n1, 1, _lib.ST_LSGAN_REAL, out, scr, 16, None), lbwd=(ptrs(a), n1, 1, _lib.ST_LSGAN_FAKE, g, ptrs(a), None))
    fns = dict(fwd=lib.st_feature_loss_forward, bwd=lib.st_feature_loss_backward, lfwd=lib.st_lsgan_loss_forward, lbwd=lib.st_lsgan_loss_backward)

    def bad(kind, **over):
        idx = dict(fwd=dict(real=0, fake=1, numels=2, n=3, out=4, scratch=5, nbytes=6),
                   bwd=dict(real=0, fake=1, numels=2, n=3, gout=4, greal=5, gfake=6),
                   lfwd=dict(x=0, numels=1, n=2, mode=3, out=4, scratch=5, nbytes=6),
                   lbwd=dict(x=0, numels=1, n=2, mode=3, gout=4, gx=5))[kind]
        args = list(ok[kind])
        for k, v in over.items():
            args[idx[k]] = v
        return fns[kind](*args)

    for kind, first in (("fwd", "real"), ("bwd", "real"), ("lfwd", "x"), ("lbwd", "x")):
        assert bad(kind, **{first: None}) == INV, kind                     # null array
        assert bad(kind, **{first: ptrs(None)}) == INV, kind               # null tensor pointer
        assert lib.st_last_error(None).decode() == "null tensor pointer"
        assert bad(kind, **{first: ptrs(a + 2)}) == INV, kind              # not 4-byte aligned
        assert bad(kind, numels=None) == INV and bad(kind, n=-1) == INV, kind
        assert bad(kind, numels=i64s(0)) == INV and bad(kind, numels=i64s(-3)) == INV, kind
    assert bad("fwd", fake=None) == INV and bad("fwd", fake=ptrs(None)) == INV and bad("fwd", out=None) == INV
    assert bad("fwd", scratch=None) == INV and bad("lfwd", scratch=None) == INV and bad("lfwd", out=None) == INV
    assert bad("fwd", nbytes=15) == INV and bad("lfwd", nbytes=8) == INV
    assert lib.st_last_error(None).decode() == "scratch is smaller than st_gan_loss_scratch_bytes() of this list"
    assert bad("fwd", numels=i64s(C + 1), nbytes=16) == INV               # two chunks need 24 bytes
    assert bad("bwd", gout=None) == INV and bad("bwd", greal=None) == INV and bad("bwd", gfake=None) == INV
    assert bad("lbwd", gout=None) == INV and bad("lbwd", gx=None) == INV
    for mode in (-1, 3):
        assert bad("lfwd", mode=mode) == INV and bad("lbwd", mode=mode) == INV
