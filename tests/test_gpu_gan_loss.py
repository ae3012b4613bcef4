"""The fused GAN losses (stabletts_amd/gan_loss.py) on the GPU, at the kernels' edges: sizes around a thread round (256), a chunk
(C = kGanLossChunk), several chunks, and more partials than stage 2 has threads; entries that start 4-byte aligned only (the second
half of an odd base, a view one float into a buffer); lists around the launch-group boundary (kGanLossMaxPairs).

The reference throughout is the same formula in torch float64 on the same fp32 inputs.  The bars come from rounding:
  |r - g| means and loss : one fp32 rounding in r - g, non-negative terms summed in fp64, one cast            -> 4 x 2^-24 relative
  LSGAN means and loss   : up to three fp32 roundings in (1 - x)^2, the same sum and cast                      -> 6 x 2^-24 relative
  gradients              : s = gout 2 / n rounded once and one product or sign, per element                   -> 2^-22 relative
Run with ``-m gpu``.
"""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu, pytest.mark.grad]

U = 2.0 ** -24
BAR_ABS, BAR_SQ, BAR_GRAD = 4 * U, 6 * U, 2.0 ** -22
DEV = "cuda:0"


@pytest.fixture(scope="module")
def G():
    from stabletts_amd import gan_loss
    return gan_loss


@pytest.fixture(scope="module")
def C(G):
    return G.chunk()


@pytest.fixture(scope="module")
def P(G):
    return G.max_pairs()


def _sizes(C):
    return [1, 2, 3, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5]


_cache = {}


def _data(n, seed):
    """Two fp32 vectors of n elements on the device, the same for every test that asks for (n, seed); never modified."""
    key = (n, seed)
    if key not in _cache:
        g = torch.Generator(device=DEV).manual_seed(1000 * seed + n % 997)
        _cache[key] = (torch.randn(n, device=DEV, generator=g), 0.5 + torch.randn(n, device=DEV, generator=g))
    return _cache[key]


def _layout(r, g, layout):
    """The same values as two tensors of their own, or as the two halves of one base (the second half 4-byte aligned only
    when the count is odd)."""
    if layout == "separate":
        return r.clone(), g.clone()
    base = torch.cat([r, g])
    return base[:r.numel()], base[r.numel():]


def _within(got, want, bar):
    got, want = (float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in (got, want))
    return abs(got - want) <= bar * abs(want)


def _feat(G, pairs):
    """(loss, means) of the feature-matching node on a flat list of pairs."""
    kinds, inputs = G._plan(pairs)
    return G._FeatureLossFn.apply(kinds, *inputs)


def _abs64(r, g):
    return (r.detach().double() - g.detach().double()).abs().mean()


def _real64(x):
    return ((1 - x.detach().double()) ** 2).mean()


def _fake64(x):
    return (x.detach().double() ** 2).mean()


def _rel_ok(got, want, bar):
    """Every element of got within bar relative of want (float64)."""
    got, want = got.detach().double(), want.double()
    return bool(((got - want).abs() <= bar * want.abs()).all())


# ---- 1. values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["separate", "halves"])
def test_single_pair_values_at_every_edge_size(G, C, layout):
    for n in _sizes(C) + [257 * C + 1]:
        r, g = _layout(*_data(n, 1), layout)
        loss, means = _feat(G, [(r, g)])
        want = _abs64(r, g)
        assert loss.dim() == 0 and means.shape == (1,)
        assert _within(means[0], want, BAR_ABS) and _within(loss, 2 * want, BAR_ABS), (n, layout, float(means[0]), float(want))
        assert torch.equal(G.feature_loss([[r]], [[g]]), loss)
        gl, gm = G.generator_loss([r])
        assert _within(gm[0], _real64(r), BAR_SQ) and _within(gl, _real64(r), BAR_SQ), (n, layout)
        dl, rl, fl = G.discriminator_loss([r], [g])
        assert _within(rl[0], _real64(r), BAR_SQ) and _within(fl[0], _fake64(g), BAR_SQ), (n, layout)
        assert _within(dl, _real64(r) + _fake64(g), BAR_SQ), (n, layout)
        assert rl[0] == float(gm[0])            # the same entry under the same op: the same bits in either list


def test_layouts_and_a_misaligned_view_give_the_same_bits(G, C):
    for n in (3, 257, C + 1, 3 * C + 5):
        r, g = _data(n, 2)
        want = _feat(G, [(r, g)])[0]
        hr, hg = _layout(r, g, "halves")
        assert hg.data_ptr() % 16 != 0 and torch.equal(_feat(G, [(hr, hg)])[0], want)
        buf = torch.empty(n + 1, device=DEV)
        buf[1:] = g
        v = buf[1:]                              # starts one float into its buffer
        assert v.data_ptr() % 16 == 4 and torch.equal(_feat(G, [(r, v)])[0], want)
        assert torch.equal(G.generator_loss([v])[0], G.generator_loss([g])[0])
        assert _within(G.generator_loss([v])[0], _real64(g), BAR_SQ)


# ---- 2. lists -----------------------------------------------------------------------------------------------------------------
def _mixed_pairs(C, count, seed):
    sizes = _sizes(C)
    return [_data(sizes[(3 * i + seed) % len(sizes)], seed + i % 7) for i in range(count)]


def test_lists_around_the_launch_boundary_match_float64(G, C, P):
    for count in (1, P, P + 1, 105):
        pairs = _mixed_pairs(C, count, 3)
        loss, means = _feat(G, pairs)
        want = [_abs64(r, g) for r, g in pairs]
        assert means.shape == (count,) and all(_within(m, w, BAR_ABS) for m, w in zip(means.tolist(), want)), count
        assert _within(loss, 2 * sum(want), BAR_ABS), count
        xs = [r for r, _ in pairs]
        gl, gm = G.generator_loss(xs)
        assert len(gm) == count and _within(gl, sum(_real64(x) for x in xs), BAR_SQ), count
        dl, rl, fl = G.discriminator_loss(xs, [g for _, g in pairs])
        assert _within(dl, sum(_real64(r) + _fake64(g) for r, g in pairs), BAR_SQ), count
        assert rl == [float(v) for v in gm]


def test_a_pairs_mean_does_not_depend_on_its_place_in_the_list(G, C, P):
    probe = _data(3 * C + 5, 9)
    alone = _feat(G, [probe])[1][0]
    alone_sq = G.generator_loss([probe[0]])[1][0]
    others = _mixed_pairs(C, 105, 4)
    for count, pos in ((P + 1, 0), (P + 1, P - 1), (P + 1, P), (P, P - 1), (105, 104), (105, 0)):
        pairs = list(others[:count])
        pairs[pos] = probe
        assert torch.equal(_feat(G, pairs)[1][pos], alone), (count, pos)
        assert torch.equal(G.generator_loss([r for r, _ in pairs])[1][pos], alone_sq), (count, pos)
    # discriminator_loss's list is r0, g0, r1, g1, ...: entry 2 i and 2 i + 1, on either side of the boundary as well
    want_r, want_g = float(alone_sq), G.discriminator_loss([probe[0]], [probe[1]])[2][0]
    for pos in (0, P // 2 - 1, P // 2, 40):
        pairs = list(others[:41])
        pairs[pos] = probe
        _, rl, fl = G.discriminator_loss([r for r, _ in pairs], [g for _, g in pairs])
        assert rl[pos] == want_r and fl[pos] == want_g, pos


# ---- 3. gradients -------------------------------------------------------------------------------------------------------------
def _planted(n, seed):
    """(r, g, positions): r == g exactly at up to 17 positions, the first and the last element among them."""
    r, g = (t.clone() for t in _data(n, seed))
    pos = torch.unique(torch.linspace(0, n - 1, min(n, 17), device=DEV).round().long())
    g[pos] = r[pos]
    return r, g, pos


@pytest.mark.parametrize("up", [1.0, 0.37])
def test_feature_loss_gradients(G, C, up):
    for n in (1, 3, 257, C + 1, 3 * C + 5):
        r, g, pos = _planted(n, 5)
        assert n < 17 or pos.numel() == 17
        r.requires_grad_(True), g.requires_grad_(True)
        (G.feature_loss([[r]], [[g]]) * up).backward()
        want_r = up * 2.0 / n * torch.sign(r.detach().double() - g.detach().double())
        assert _rel_ok(r.grad, want_r, BAR_GRAD) and _rel_ok(g.grad, -want_r, BAR_GRAD), n
        assert torch.equal(r.grad, -g.grad), n
        assert bool((r.grad[pos] == 0).all()) and bool((g.grad[pos] == 0).all()), n       # sign(0) = 0, as torch's abs'
        if n > 17:
            assert int((r.grad == 0).sum()) == 17
    # one side only: a gradient for that side only
    r, g, _ = _planted(C + 1, 6)
    r.requires_grad_(True)
    (G.feature_loss([[r]], [[g]]) * up).backward()
    assert g.grad is None and _rel_ok(r.grad, up * 2.0 / r.numel() * torch.sign(r.detach().double() - g.double()), BAR_GRAD)
    r2, g2, _ = _planted(C + 1, 6)
    g2.requires_grad_(True)
    (G.feature_loss([[r2]], [[g2]]) * up).backward()
    assert r2.grad is None and torch.equal(g2.grad, -r.grad)


@pytest.mark.parametrize("up", [1.0, 0.37])
@pytest.mark.parametrize("count", [1, 3, 5, 8])
def test_discriminator_and_generator_loss_values_and_gradients(G, count, up):
    shapes = [(2, 1), (2, 7), (3, 1, 5, 9)]
    gen = torch.Generator(device=DEV).manual_seed(70 + count)
    dr = [torch.randn(shapes[i % 3], device=DEV, generator=gen).requires_grad_(True) for i in range(count)]
    dg = [torch.randn(shapes[i % 3], device=DEV, generator=gen).requires_grad_(True) for i in range(count)]
    out = G.discriminator_loss(dr, dg)
    assert isinstance(out, tuple) and len(out) == 3
    loss, r_losses, g_losses = out
    assert loss.dim() == 0 and len(r_losses) == len(g_losses) == count and all(type(v) is float for v in r_losses + g_losses)
    assert all(float(np.float32(v)) == v for v in r_losses + g_losses)          # fp32 means, read as floats
    assert all(_within(v, _real64(t), BAR_SQ) for v, t in zip(r_losses, dr)) and all(_within(v, _fake64(t), BAR_SQ) for v, t in zip(g_losses, dg))
    assert _within(loss, sum(_real64(a) + _fake64(b) for a, b in zip(dr, dg)), BAR_SQ)
    (loss * up).backward()
    for t in dr:
        assert t.grad.shape == t.shape and _rel_ok(t.grad, up * 2.0 * (t.detach().double() - 1) / t.numel(), BAR_GRAD)
    for t in dg:
        assert _rel_ok(t.grad, up * 2.0 * t.detach().double() / t.numel(), BAR_GRAD)

    xs = [t.detach().clone().requires_grad_(True) for t in dg]
    out = G.generator_loss(xs)
    assert isinstance(out, tuple) and len(out) == 2
    loss, gen_losses = out
    assert loss.dim() == 0 and len(gen_losses) == count and all(v.dim() == 0 and not v.requires_grad for v in gen_losses)
    assert all(_within(v, _real64(t), BAR_SQ) for v, t in zip(gen_losses, xs)) and _within(loss, sum(_real64(t) for t in xs), BAR_SQ)
    (loss * up).backward()
    for t in xs:
        assert _rel_ok(t.grad, up * 2.0 * (t.detach().double() - 1) / t.numel(), BAR_GRAD)
    # a non-contiguous logit tensor is made contiguous and gets its gradient in its own shape
    nc = torch.randn(7, 4, device=DEV, generator=gen).t().requires_grad_(True)
    lnc, _ = G.generator_loss([nc])
    lnc.backward()
    assert _within(lnc, _real64(nc), BAR_SQ) and _rel_ok(nc.grad, 2.0 * (nc.detach().double() - 1) / nc.numel(), BAR_GRAD)


# ---- 4. halves of one base against the general path ---------------------------------------------------------------------------
@pytest.mark.parametrize("up", [1.0, 0.37])
def test_halves_path_and_general_path_give_the_same_bits(G, C, up):
    for n in (3, 257, C + 1, 3 * C + 5):
        r0, g0, _ = _planted(n, 7)
        r, g = r0.clone().requires_grad_(True), g0.clone().requires_grad_(True)
        base = torch.cat([r0, g0]).requires_grad_(True)
        assert G._halves_base(base[:n], base[n:]) is base and G._halves_base(r, g) is None
        lg = G.feature_loss([[r]], [[g]])
        lh = G.feature_loss([[base[:n]]], [[base[n:]]])
        assert torch.equal(lg, lh), n
        (lg * up).backward(), (lh * up).backward()
        assert torch.equal(base.grad, torch.cat([r.grad, g.grad])), n
        r, g = r0.clone().requires_grad_(True), g0.clone().requires_grad_(True)
        base.grad = None
        lg, rl_g, fl_g = G.discriminator_loss([r], [g])
        lh, rl_h, fl_h = G.discriminator_loss([base[:n]], [base[n:]])
        assert torch.equal(lg, lh) and rl_g == rl_h and fl_g == fl_h, n
        (lg * up).backward(), (lh * up).backward()
        assert torch.equal(base.grad, torch.cat([r.grad, g.grad])), n
        assert _rel_ok(base.grad, up * 2.0 * torch.cat([r0.double() - 1, g0.double()]) / n, BAR_GRAD), n


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------
def test_two_runs_of_a_65_pair_list_agree_bit_for_bit(G, C):
    def run():
        pairs = [(r.clone().requires_grad_(True), g.clone().requires_grad_(True)) for r, g in _mixed_pairs(C, 65, 8)]
        loss, means = _feat(G, pairs)
        (loss * 0.37).backward()
        dl, rl, fl = G.discriminator_loss([r.detach() for r, _ in pairs], [g.detach() for _, g in pairs])
        return [loss.detach(), means, dl] + [t.grad for p in pairs for t in p], rl + fl
    (ta, fa), (tb, fb) = run(), run()
    assert fa == fb and all(torch.equal(a, b) for a, b in zip(ta, tb))


# ---- 6. the discriminators' own maps -------------------------------------------------------------------------------------------
def _torch_feature(fmap_rs, fmap_gs):
    return 2 * sum(torch.mean(torch.abs(rl - gl)) for dr, dg in zip(fmap_rs, fmap_gs) for rl, gl in zip(dr, dg))


def _torch_disc(y_d_rs, y_d_gs):
    return sum(torch.mean((1 - dr) ** 2) + torch.mean(dg ** 2) for dr, dg in zip(y_d_rs, y_d_gs))


def _torch_gen(y_d_gs):
    return sum(torch.mean((1 - dg) ** 2) for dg in y_d_gs)


def _modules():
    from stabletts_amd.discriminator import MultiPeriodDiscriminator, MultiResolutionDiscriminator
    from tests import mpd_restatement as RP
    from tests import mrd_restatement as RR
    mpd = MultiPeriodDiscriminator((2, 3))
    mpd.load_state_dict({k: torch.from_numpy(v) for k, v in RP.make_mpd_state_dict(21, (2, 3)).items()}, strict=True)
    mrd = MultiResolutionDiscriminator((64, 32))
    mrd.load_state_dict({k: torch.from_numpy(v) for k, v in RR.with_windows(RR.make_mrd_state_dict(22, (64, 32)), (64, 32)).items()}, strict=True)
    return RP, [("mpd", mpd.to(DEV).train(), 99), ("mrd", mrd.to(DEV).train(), 97)]


def test_integration_at_the_discriminators_smallest_shapes(G):
    """One forward of each native discriminator; the three losses natively and as torch expressions, differentiated with respect
    to the map tensors the discriminator produced (the bases the returned halves are views of: a base's gradient is the two
    halves' gradients side by side, elementwise comparable between the paths), then a backward through the modules for d y_hat.
    Figures of the last run: profiles/gan_loss_parity.txt."""
    RP, mods = _modules()
    for name, m, T in mods:
        y = torch.from_numpy(RP.make_audio(2, T, 31)).to(DEV)
        yh_np = RP.make_audio(2, T, 32)
        yh = torch.from_numpy(yh_np).to(DEV).requires_grad_(True)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = m(y, yh)
        bases = []
        for t in [f for d in fmap_rs for f in d]:
            assert t._base is not None
            bases.append(t._base)
        as64 = lambda nested: [[t.double() for t in d] if isinstance(d, list) else d.double() for d in nested]      # noqa: E731
        for what, native, plain, plain64 in (
                ("feature", lambda: G.feature_loss(fmap_rs, fmap_gs), lambda: _torch_feature(fmap_rs, fmap_gs), lambda: _torch_feature(as64(fmap_rs), as64(fmap_gs))),
                ("disc", lambda: G.discriminator_loss(y_d_rs, y_d_gs)[0], lambda: _torch_disc(y_d_rs, y_d_gs), lambda: _torch_disc(as64(y_d_rs), as64(y_d_gs))),
                ("gen", lambda: G.generator_loss(y_d_gs)[0], lambda: _torch_gen(y_d_gs), lambda: _torch_gen(as64(y_d_gs)))):
            wrt = bases if what == "feature" else [b for b in bases if any(b is t._base for t in y_d_rs)]
            assert len(wrt) == (len(bases) if what == "feature" else len(y_d_rs))
            # the float64 expressions' gradient: differentiate in float64 with respect to float64 copies of the bases
            b64 = [b.detach().double().requires_grad_(True) for b in wrt]
            n = y.shape[0]
            if what == "feature":
                l64 = 2 * sum(torch.mean(torch.abs(b[:n] - b[n:])) for b in b64)
            elif what == "disc":
                l64 = sum(torch.mean((1 - b[:n]) ** 2) + torch.mean(b[n:] ** 2) for b in b64)
            else:
                l64 = sum(torch.mean((1 - b[n:]) ** 2) for b in b64)
            g64 = torch.autograd.grad(l64, b64)
            ln, lp = native(), plain()
            assert _within(ln, l64, BAR_ABS if what == "feature" else BAR_SQ), (name, what)
            gn = torch.autograd.grad(ln, wrt, retain_graph=True)
            gp = torch.autograd.grad(lp, wrt, retain_graph=True)
            worst = [max(float(((a.double() - w).abs() / w.abs().clamp_min(1e-300)).max()) for a, w in zip(gs, g64)) for gs in (gn, gp)]
            print(f"{name} {what}: loss native {float(ln.detach()):.9g} torch {float(lp.detach()):.9g} float64 {float(l64.detach()):.12g}; worst elementwise relative "
                  f"gradient error native {worst[0]:.3e} torch {worst[1]:.3e} (bar {BAR_GRAD:.3e})")
            for a, p, w in zip(gn, gp, g64):
                assert a.shape == w.shape and _rel_ok(a, w, BAR_GRAD) and _rel_ok(p, w, BAR_GRAD), (name, what)

        # d y_hat through the module: native loss lines, torch expressions, and the expressions on .double() copies of the maps
        def dyhat(lines):
            m.zero_grad(set_to_none=True)
            x = torch.from_numpy(yh_np).to(DEV).requires_grad_(True)
            lines(*m(y, x)).backward()
            return x.grad.detach().double().cpu().numpy()
        d_native = dyhat(lambda rs, gs, fr, fg: G.discriminator_loss(rs, gs)[0] + G.feature_loss(fr, fg) + G.generator_loss(gs)[0])
        d_torch = dyhat(lambda rs, gs, fr, fg: _torch_disc(rs, gs) + _torch_feature(fr, fg) + _torch_gen(gs))
        d_64 = dyhat(lambda rs, gs, fr, fg: _torch_disc(as64(rs), as64(gs)) + _torch_feature(as64(fr), as64(fg)) + _torch_gen(as64(gs)))
        yard, dist = RP.rel_l2(d_torch, d_64), RP.rel_l2(d_native, d_64)
        print(f"{name} d y_hat: relative L2 to the float64-lines path: native {dist:.3e}, torch expressions {yard:.3e} (bar 4 x = {4 * yard:.3e})")
        if yard == 0.0:
            assert np.array_equal(d_native, d_64), (name, dist)
        else:
            assert dist <= 4 * yard, (name, dist, yard)
