"""The native multi-resolution discriminator (stabletts_amd/discriminator.py) on the GPU: forward and gradients against float64
-- the REAL reference module's (tests/golden/mrd_grads.npz) and, at shapes the fixture lacks, the torch restatement's
(tests/mrd_restatement.py, pinned to the real module by tests/test_mrd_cpu.py) -- determinism and independence, the module rules
and a short AdamW trajectory against torch autograd of the restatement.

Metric: relative L2 distance per tensor (over the stored elements where the fixture is the reference).  Bars: 4 x torch fp32's own
distance from float64 for that tensor -- the fixture's err32 / fmap_err32, or, in the shape sweep, the restatement run in fp32 on
the CPU at the same branch pattern.  Gradients in training mode are compared SIGN-CONSISTENTLY (see mpd_restatement) wherever the
reference is not the fixture's sign-clean train step: the float64 side is evaluated at the branch pattern the native forward took
(layers 1..4 from the returned maps, layer 0 from st_debug_capture), after asserting that this pattern differs from float64's own
only where the float64 value is within the forward bar of zero.  Every figure is printed beside its bar.  Run with ``-m gpu``.
"""
import os

import numpy as np
import pytest
import torch

from tests import mrd_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu, pytest.mark.grad]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mrd_grads.npz")))


def _dr(W, sd_np, slope=0.1):
    from stabletts_amd.discriminator import DiscriminatorR
    d = DiscriminatorR(W)
    d.lrelu_slope = slope
    d.load_state_dict({k: torch.from_numpy(v) for k, v in R.with_windows(sd_np, W).items()}, strict=True)
    return d.to("cuda:0").train()


def _mrd(sd_np, fft_sizes=R.FFT_SIZES):
    from stabletts_amd.discriminator import MultiResolutionDiscriminator
    m = MultiResolutionDiscriminator(fft_sizes)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.with_windows(sd_np, fft_sizes).items()}, strict=True)
    return m.to("cuda:0").train()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _grads(mod):
    return {n: _np(p.grad) for n, p in mod.named_parameters()}


def _torch_losses(y_d_rs, y_d_gs, fmap_rs, fmap_gs):
    """discriminator_loss + feature_loss + generator_loss (loss.py:37-66) on the returned tensors."""
    disc = sum(torch.mean((1 - dr) ** 2) + torch.mean(dg ** 2) for dr, dg in zip(y_d_rs, y_d_gs))
    feat = 2 * sum(torch.mean(torch.abs(rl - gl)) for dr, dg in zip(fmap_rs, fmap_gs) for rl, gl in zip(dr, dg))
    gen = sum(torch.mean((1 - dg) ** 2) for dg in y_d_gs)
    return disc + feat + gen


def _captured_forward(d, x):
    """d(x) with layer 0's post-activations captured: (logits, fmap, [band] layer-0 activation on the CPU)."""
    eng = d.engine()
    eng.debug_capture(True)
    logits, fmap = d(x)
    B = x.shape[0]
    a0 = [torch.from_numpy(eng.debug_fetch(f"band_convs.{c}.0.act").astype(np.float64)).view(B, 32, -1, hi - lo) for c, (lo, hi) in enumerate(d.bands)]
    eng.debug_capture(False)
    return logits, fmap, a0


def _native_signs(fmap, a0):
    """[band][layer] pre > 0 as the native forward took it: the sign of the post-activation (slope > 0 keeps it)."""
    return [[a0[c] > 0] + [fmap[4 * c + i].detach().cpu() > 0 for i in range(4)] for c in range(5)]


def _assert_signs_are_float64s_up_to_rounding(signs, own, tols):
    """The native branch pattern differs from float64's own only where the float64 post-activation is within tols[band][layer] of 0."""
    flips = 0
    for c in range(5):
        vals = [own.acts0[c]] + [own.fmaps[4 * c + i].detach() for i in range(4)]
        for i in range(5):
            diff = signs[c][i] != own.signs[c][i]
            assert bool((vals[i][diff].abs() <= tols[c][i]).all()), (c, i, float(vals[i][diff].abs().max()), tols[c][i])
            flips += int(diff.sum())
    return flips


def _yardsticks(g32, g64):
    """Torch fp32's distance from float64 per parameter tensor, the yardstick of the native gradients (bar: 4 x).  Every tensor of
    more than one element -- the v's, the 32-element g's and biases -- is measured against its own distance.  The two scalars
    (conv_post's g and bias) cannot be: one draw of a scalar's rounding error can land anywhere below fp32's resolution
    (conv_post.bias at (512, 1, 700): 1.5e-09, a 40th of 2^-24).  They are measured against like quantities: the pooled relative
    L2 distance of all tensors of their kind (the 26 g's, the 26 biases, their own included: the same sums over the same
    activations, one layer up), or their own distance where that is larger (an ill-conditioned scalar that torch, too, misses by
    more)."""
    own = {n: R.rel_l2(g32[n], g64[n]) for n in g64}
    out = dict(own)
    for kind in ("original0", "bias"):
        like = [n for n in g64 if n.endswith(kind)]
        pooled = R.rel_l2(np.concatenate([g32[n].reshape(-1) for n in like]), np.concatenate([g64[n].reshape(-1) for n in like]))
        for n in like:
            if g64[n].size == 1:
                out[n] = max(own[n], pooled)
    return out


# ---- 1. forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.LINEAR_CASES))
def test_forward_linear_cases_against_the_real_module(gold, case):
    W, B, T, wseed, aseed = R.LINEAR_CASES[case]
    d = _dr(W, R.make_dr_state_dict(wseed), 1.0)
    with torch.no_grad():
        logits, fmap = d(torch.from_numpy(R.make_audio(B, T, aseed)).cuda())
    assert len(fmap) == 21 and logits is fmap[-1] and logits.dim() == 4
    assert [",".join(map(str, f.shape)) for f in fmap] == gold[case + "/fmap_shapes"].tolist()
    fails = []
    for i, f in enumerate(fmap):
        err, bar = R.rel_l2(R.stored(1000 + i, _np(f), wseed), gold[f"{case}/fmap/{i}"]), 4 * float(gold[case + "/fmap_err32"][i])
        print(f"{case} fmap {i:2d}: {err:.2e} (bar {bar:.2e})")
        if err > bar:
            fails.append(i)
    assert not fails, fails


def test_forward_train_step_against_the_real_module(gold):
    seed = int(gold["train_step/seed"].reshape(-1)[0])
    B, T = R.TRAIN_STEP["B"], R.TRAIN_STEP["T"]
    m = _mrd(R.make_mrd_state_dict(seed))
    y, yh = torch.from_numpy(R.make_audio(B, T, seed + 1)).cuda(), torch.from_numpy(R.make_audio(B, T, seed + 2)).cuda()
    with torch.no_grad():
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = m(y, yh)
    fails = []
    for k, W in enumerate(R.FFT_SIZES):
        for i in range(21):
            f = torch.cat([fmap_rs[k][i], fmap_gs[k][i]])
            err = R.rel_l2(R.stored(2000 + 100 * k + i, _np(f), seed), gold[f"train_step/fmap/{k}/{i}"])
            bar = 4 * float(gold["train_step/fmap_err32"][k][i])
            print(f"train_step W={W} fmap {i:2d}: {err:.2e} (bar {bar:.2e})")
            if err > bar:
                fails.append((k, i))
        err = R.rel_l2(_np(torch.cat([y_d_rs[k], y_d_gs[k]])), gold[f"train_step/logits/{k}"])
        bar = 4 * float(gold["train_step/fmap_err32"][k][20])
        print(f"train_step W={W} logits: {err:.2e} (bar {bar:.2e})")
        if err > bar:
            fails.append((k, "logits"))
    assert not fails, fails


# ---- 2. gradients against the fixture --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.LINEAR_CASES))
def test_gradients_linear_cases_against_the_real_module(gold, case):
    W, B, T, wseed, aseed = R.LINEAR_CASES[case]
    d = _dr(W, R.make_dr_state_dict(wseed), 1.0)
    x = torch.from_numpy(R.make_audio(B, T, aseed)).cuda().requires_grad_(True)
    _, fmap = d(x)
    R.linear_loss(fmap, wseed).backward()
    grads, dx = _grads(d), _np(x.grad)
    names = gold[case + "/names"].tolist()
    assert list(grads) == names
    fails = []
    for i, n in enumerate(names):
        err, own = R.rel_l2(R.stored(i, grads[n], wseed), gold[f"{case}/grad/{n}"]), float(gold[case + "/err32"][i])
        print(f"{case} {n:56s} native {err:.2e}  torch fp32 {own:.2e}  ratio {err / own:5.2f} (bar 4)")
        if err > 4 * own:
            fails.append(n)
    err, own = R.rel_l2(dx, gold[case + "/dx64"]), float(gold[case + "/dx_err32"].reshape(-1)[0])
    print(f"{case} d x: native {err:.2e}  torch fp32 {own:.2e}  ratio {err / own:5.2f} (bar 4)")
    assert not fails and err <= 4 * own, fails


def test_gradients_train_step_against_the_real_module(gold):
    """The fixture's train step is sign-clean between torch's fp32 and float64 runs, so the native gradients are compared with the
    stored float64 ones directly."""
    seed = int(gold["train_step/seed"].reshape(-1)[0])
    B, T = R.TRAIN_STEP["B"], R.TRAIN_STEP["T"]
    m = _mrd(R.make_mrd_state_dict(seed))
    y, yh = torch.from_numpy(R.make_audio(B, T, seed + 1)).cuda(), torch.from_numpy(R.make_audio(B, T, seed + 2)).cuda().requires_grad_(True)
    _torch_losses(*m(y, yh)).backward()
    grads, dyh = _grads(m), _np(yh.grad)
    names = gold["train_step/names"].tolist()
    assert list(grads) == names
    fails = []
    for i, n in enumerate(names):
        err, own = R.rel_l2(R.stored(i, grads[n], seed), gold[f"train_step/grad/{n}"]), float(gold["train_step/err32"][i])
        print(f"train_step {n:72s} native {err:.2e}  torch fp32 {own:.2e}  ratio {err / own:5.2f} (bar 4)")
        if err > 4 * own:
            fails.append(n)
    err, own = R.rel_l2(dyh, gold["train_step/dyhat64"]), float(gold["train_step/dyhat_err32"].reshape(-1)[0])
    print(f"train_step d y_hat: native {err:.2e}  torch fp32 {own:.2e}  ratio {err / own:5.2f} (bar 4)")
    assert not fails and err <= 4 * own, fails


# ---- 3. the shape sweep against the float64 restatement ----------------------------------------------------------------------
# (window, B, T): the smallest shapes that exercise each path
SWEEP = [
    (32, 2, 17),          # T just above W / 2, 3 frames, band widths 1 / 3 / 4 / 4 / 5
    (32, 2, 97),
    (64, 3, 96), (64, 3, 97),      # T a multiple of the hop and not; widths 3 / 5 / 8 / 8 / 9: odd and even widths at every stride-2 layer
    (128, 2, 331),
    (512, 1, 700),        # widths 25 / 39 / 64 / 64 / 65: a column tile exactly full and one over
    (2048, 1, 1100),      # the largest FFT, widths up to 257
]


def _restated(sd_np, x_np, W, wseed, dtype, signs):
    sd = R.to_torch(sd_np, dtype=dtype, requires_grad=True)
    x = torch.from_numpy(x_np).to(dtype).requires_grad_(True)
    out = R.forward(sd, x, W, signs=signs)
    R.linear_loss(out.fmaps, wseed).backward()
    return [f.detach().double().numpy() for f in out.fmaps], {n: t.grad.double().numpy() for n, t in sd.items()}, x.grad.double().numpy()


@pytest.mark.parametrize("W,B,T", SWEEP)
def test_forward_and_gradients_across_the_shape_sweep(W, B, T):
    """Slope 0.1 and the linear loss sum(fmap * W) over all 21 maps, against the float64 restatement at the native branch pattern.
    Yardstick: the restatement in fp32 on the CPU at the same pattern -- per feature map, for d x, and per parameter tensor
    (_yardsticks: each tensor's own distance from float64; the two scalars against the tensors of their kind).  The bar is 4 x the
    yardstick throughout."""
    wseed, aseed = 400 + W, 500 + T
    sd_np, x_np = R.make_dr_state_dict(wseed), R.make_audio(B, T, aseed)
    d = _dr(W, sd_np)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    _, fmap, a0 = _captured_forward(d, x)
    R.linear_loss(fmap, wseed).backward()
    fm, grads, dx = [_np(f) for f in fmap], _grads(d), _np(x.grad)
    signs = _native_signs(fmap, a0)
    # float64 and torch fp32 (CPU) at the native branch pattern; float64 at its own for the sign check
    rf, rg, rdx = _restated(sd_np, x_np, W, wseed, torch.float64, signs)
    tf, tg, tdx = _restated(sd_np, x_np, W, wseed, torch.float32, signs)
    assert [f.shape for f in fm] == [f.shape for f in rf]
    fbar = [4 * R.rel_l2(a, b) for a, b in zip(tf, rf)]
    with torch.no_grad():
        own = R.forward(R.to_torch(sd_np), torch.from_numpy(x_np).double(), W)
    tols = [[max(fbar[4 * c:4 * c + 4]) * float(own.acts0[c].norm())] + [fbar[4 * c + i] * float(own.fmaps[4 * c + i].norm()) for i in range(4)]
            for c in range(5)]
    flips = _assert_signs_are_float64s_up_to_rounding(signs, own, tols)
    fails = []
    ferr = [R.rel_l2(a, b) for a, b in zip(fm, rf)]
    for i, (e, bar) in enumerate(zip(ferr, fbar)):
        if e > bar:
            fails.append(("fmap", i, e, bar))
    yards = _yardsticks(tg, rg)
    worst = (0.0, None)
    for n in rg:
        err, yard = R.rel_l2(grads[n], rg[n]), yards[n]
        worst = max(worst, (err / yard, n))
        if err > 4 * yard:
            fails.append((n, err, yard))
    de, dbar = R.rel_l2(dx, rdx), 4 * R.rel_l2(tdx, rdx)
    print(f"W={W} B={B} T={T}: {flips} branch flips against float64's own signs; fmaps worst ratio to bar {max(e / b for e, b in zip(ferr, fbar)):.2f}; "
          f"worst parameter {worst[1]} ratio {worst[0]:.2f} (bar 4); d x {de:.2e} (bar {dbar:.2e})")
    assert not fails and de <= dbar, fails


def test_sweep_runs_weight_gradients_with_one_split_k_plane_and_with_several():
    counts = {}
    for W, B, T in SWEEP:
        eng = _dr(W, R.make_dr_state_dict(1)).engine()
        for c in range(5):
            for i in range(5):
                n = eng.resolution_disc_wgrad_planes(B, T, c, i)
                counts[n] = counts.get(n, 0) + 1
    print("weight-gradient launches of the sweep by split-K planes:", dict(sorted(counts.items())))
    assert counts.get(1, 0) > 0 and sum(v for k, v in counts.items() if k > 1) > 0


# ---- 4. determinism and independence ---------------------------------------------------------------------------------------
def test_determinism_and_independence():
    from stabletts_amd.discriminator import DiscriminatorR
    seed, B, T, sizes = 601, 3, 700, (512, 128, 32)
    sd_np, y_np, yh_np = R.make_mrd_state_dict(seed, sizes), R.make_audio(B, T, seed + 1), R.make_audio(B, T, seed + 2)
    m = _mrd(sd_np, sizes)

    def step():
        m.zero_grad(set_to_none=True)
        y, yh = torch.from_numpy(y_np).cuda(), torch.from_numpy(yh_np).cuda().requires_grad_(True)
        out = m(y, yh)
        _torch_losses(*out).backward()
        return out, {n: p.grad.clone() for n, p in m.named_parameters()}, yh.grad.clone()

    (a_rs, a_gs, a_fr, a_fg), ga, da = step()
    (b_rs, b_gs, b_fr, b_fg), gb, db = step()
    assert torch.equal(da, db) and all(torch.equal(ga[n], gb[n]) for n in ga)
    assert all(torch.equal(u, v) for fa, fb in ((a_fr, b_fr), (a_fg, b_fg)) for la, lb in zip(fa, fb) for u, v in zip(la, lb))
    # the halves of mrd(y, y_hat) are DiscriminatorR(y) and DiscriminatorR(y_hat) alone; an item alone is its rows of the batch
    with torch.no_grad():
        y, yh = torch.from_numpy(y_np).cuda(), torch.from_numpy(yh_np).cuda()
        for k, d in enumerate(m.discriminators):
            assert isinstance(d, DiscriminatorR)
            lr, fr = d(y)
            lg, fg = d(yh)
            assert torch.equal(lr, a_rs[k]) and torch.equal(lg, a_gs[k])
            assert all(torch.equal(u, v) for u, v in zip(fr, a_fr[k])) and all(torch.equal(u, v) for u, v in zip(fg, a_fg[k]))
            l1, f1 = d(y[1:2])
            assert torch.equal(l1, lr[1:2]) and all(torch.equal(u, v[1:2]) for u, v in zip(f1, fr))


# ---- 5. module rules -------------------------------------------------------------------------------------------------------
def test_module_rules():
    from stabletts_amd import _lib
    seed, B, T, sizes = 701, 2, 331, (128, 64)
    m = _mrd(R.make_mrd_state_dict(seed, sizes), sizes)
    y, yh = torch.from_numpy(R.make_audio(B, T, seed + 1)).cuda(), torch.from_numpy(R.make_audio(B, T, seed + 2)).cuda()

    def flat(out):
        return [t for part in out for item in part for t in (item if isinstance(item, list) else [item])]

    # no_grad / eval: the keep-nothing forward, bitwise the training forward's values
    train_out = flat(m(y, yh))
    assert all(t.requires_grad for t in train_out)
    with torch.no_grad():
        ng = flat(m(y, yh))
    ev = flat(m.eval()(y, yh))
    m.train()
    assert not any(t.requires_grad for t in ng + ev)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(train_out, ng, ev))
    assert all(d.engine().train_serial() == 1 for d in m.discriminators)       # the two other calls kept nothing and dropped nothing

    def leg(mod, fake):
        mod.zero_grad(set_to_none=True)
        _torch_losses(*mod(y, fake)).backward()
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in mod.named_parameters()}

    # y_hat.detach(): no d y_hat, parameter gradients bitwise those of the attached run
    fake = yh.clone().requires_grad_(True)
    attached = leg(m, fake)
    d_attached = fake.grad.clone()
    det = fake.detach()
    detached = leg(m, det)
    assert det.grad is None and all(torch.equal(attached[n], detached[n]) for n in attached)
    # a frozen module: d y_hat bitwise that of the unfrozen run, no parameter gradient
    m.requires_grad_(False)
    fake2 = yh.clone().requires_grad_(True)
    frozen = leg(m, fake2)
    assert all(g is None for g in frozen.values()) and torch.equal(fake2.grad, d_attached)
    m.requires_grad_(True)
    leg(m, yh)
    assert all(p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all() for p in m.parameters())
    # a second backward through the same forward, and a backward after another forward, are refused
    d = m.discriminators[0]
    x = torch.cat([y, yh])
    logits, _ = d(x)
    logits.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="differentiated already"):
        logits.sum().backward()
    logits, _ = d(x)
    d(x)
    with pytest.raises(RuntimeError, match="activations are gone"):
        logits.sum().backward()
    logits, _ = d(x)
    torch.optim.SGD(d.parameters(), lr=1e-2).step()              # a parameter update between forward and backward
    with pytest.raises(RuntimeError, match="activations are gone"):
        logits.sum().backward()
    # T <= window_length // 2 raises (the reference's reflect padding raises there too)
    with pytest.raises(ValueError, match="too short"):
        d(torch.zeros(1, 1, 64, device="cuda"))
    with torch.no_grad():
        assert d(torch.zeros(1, 1, 65, device="cuda"))[0].shape == (1, 1, 3, 10)
    # the C ABI: bad sizes, null pointers, a backward that is not the held forward's, a handle of another kind
    import ctypes
    eng, lib = d.engine(), _lib.load()
    xs = x.contiguous()
    fm = [torch.full(s, 7.0, device="cuda") for s in eng.resolution_disc_fmap_shapes(2 * B, T)]
    dx = torch.full((2 * B, 1, T), 7.0, device="cuda")
    gflat = torch.full((eng.grad_layout()[None],), 7.0, device="cuda")
    ptrs = (ctypes.c_void_p * 21)(*[f.data_ptr() for f in fm])
    holed = (ctypes.c_void_p * 21)(*[f.data_ptr() for f in fm[:20]], None)
    for fwd in (lib.st_resolution_disc_forward, lib.st_resolution_disc_train_forward):
        assert fwd(eng.handle, xs.data_ptr(), ptrs, 0, T, None) == _lib.ST_ERR_INVALID
        assert fwd(eng.handle, xs.data_ptr(), ptrs, 2 * B, 0, None) == _lib.ST_ERR_INVALID
        assert fwd(eng.handle, xs.data_ptr(), ptrs, 2 * B, 64, None) == _lib.ST_ERR_INVALID       # T <= window_length / 2
        assert fwd(eng.handle, None, ptrs, 2 * B, T, None) == _lib.ST_ERR_INVALID
        assert fwd(eng.handle, xs.data_ptr(), None, 2 * B, T, None) == _lib.ST_ERR_INVALID
        assert fwd(eng.handle, xs.data_ptr(), holed, 2 * B, T, None) == _lib.ST_ERR_INVALID
        assert fwd(eng.handle, xs.data_ptr(), ptrs, 1 << 20, T, None) == _lib.ST_ERR_INVALID
    assert lib.st_resolution_disc_train_backward(eng.handle, None, dx.data_ptr(), gflat.data_ptr(), 2 * B, T, None) == _lib.ST_ERR_INVALID
    eng.finalize()                                               # drops the held activations
    assert eng.train_serial() == 0
    assert lib.st_resolution_disc_train_backward(eng.handle, ptrs, dx.data_ptr(), gflat.data_ptr(), 2 * B, T, None) == _lib.ST_ERR_STATE
    assert b"st_resolution_disc_train_forward" in lib.st_last_error(eng.handle)
    assert lib.st_resolution_disc_train_forward(eng.handle, xs.data_ptr(), ptrs, 2 * B, T, None) == _lib.ST_OK
    assert eng.train_serial() > 0
    torch.cuda.synchronize()
    assert all(torch.isfinite(f).all() and not torch.all(f == 7.0) for f in fm)
    assert lib.st_resolution_disc_train_backward(eng.handle, ptrs, dx.data_ptr(), gflat.data_ptr(), 2 * B, T - 1, None) == _lib.ST_ERR_STATE
    assert lib.st_resolution_disc_train_backward(eng.handle, ptrs, dx.data_ptr(), gflat.data_ptr(), B, T, None) == _lib.ST_ERR_STATE
    pd = _lib.Engine(0, 0, 0, 0, 0, 0, 0, "f16", 0, period_discriminator=dict(period=3, lrelu_slope=0.1))       # a handle of another kind
    assert lib.st_resolution_disc_train_forward(pd.handle, xs.data_ptr(), ptrs, 2 * B, T, None) == _lib.ST_ERR_STATE
    assert lib.st_resolution_disc_train_backward(pd.handle, ptrs, dx.data_ptr(), gflat.data_ptr(), 2 * B, T, None) == _lib.ST_ERR_STATE
    assert lib.st_period_disc_train_forward(eng.handle, xs.data_ptr(), ptrs, 2 * B, T, None) == _lib.ST_ERR_STATE
    pd.close()
    torch.cuda.synchronize()
    assert torch.all(dx == 7.0) and torch.all(gflat == 7.0)      # the error paths left the output buffers untouched


# ---- 6. trajectory ---------------------------------------------------------------------------------------------------------
def test_discriminator_leg_trajectory_against_torch_autograd(gold):
    """Three AdamW steps of the discriminator leg (vocoders/vocos/train.py:74,98-110: lr 1e-4, mrd(y, y_hat.detach()),
    discriminator_loss) of the default model at B = 2, T = 2100 on the native module, with torch autograd of the restatement in
    fp32 (CPU) alongside: at every step the restatement is evaluated at the parameters the native optimizer has reached and at the
    branch pattern the native forward took.  (The torch side takes the native parameters rather than its own AdamW's: AdamW's first
    steps move every element by +-lr whatever its size, so one near-zero gradient element whose rounding differs between the two
    sides would put 2 lr between them, and the later steps would measure that instead of the kernels.)  The bars are the sweep's:
    the same restatement in float64 is the reference, and every step's native parameter gradients stay within 4 x the fp32
    restatement's own distance from it, per tensor (_yardsticks; the six scalars against the tensors of their kind); the loss within 2 x 4 x the fixture's fmap_err32 of the logits (a mean of squares doubles a relative error).
    This is the check that in-place parameter binding and the weight re-norm after an optimizer step work: a native forward on
    stale weights differs from the restatement at the stepped ones by ~1e-3, thousands of bars.
    A second torch side IS stepped alongside with its own AdamW from the same start (at the native branch pattern).  Against it
    the bars are those such a comparison supports: the loss within 1e-3 at every step (test_gpu_mpd's bar for the same
    comparison), and after the three steps all 1,413,990 parameters as one vector within 1e-4 relative L2 -- an element whose
    update sign differs is 2 lr = 2e-4 apart on a vector of norm ~70, 3e-6 each, so hundreds may differ, while one (3, 9) weight
    tensor stepped the wrong way (27,648 elements, 6e-4 each) would give 1.4e-3."""
    seed, B, T, steps = 801, R.TRAIN_STEP["B"], R.TRAIN_STEP["T"], 3
    sd_np = R.make_mrd_state_dict(seed)
    y_np, yh_np = R.make_audio(B, T, seed + 1), R.make_audio(B, T, seed + 2)
    x = torch.cat([torch.from_numpy(y_np), torch.from_numpy(yh_np)]).cuda()
    xc = x.cpu()
    m = _mrd(sd_np)
    opt_n = torch.optim.AdamW(m.parameters(), lr=1e-4)
    lbar = 2 * 4 * float(gold["train_step/fmap_err32"][:, 20].max())

    def restated(params, signs, dtype):
        sd = {n: t.detach().to(dtype).clone().requires_grad_(True) for n, t in params.items()}
        loss = 0
        for k, W in enumerate(R.FFT_SIZES):
            lg = R.forward(sd, xc.to(dtype), W, signs=signs[k], prefix=f"discriminators.{k}.").fmaps[-1]
            loss = loss + torch.mean((1 - lg[:B]) ** 2) + torch.mean(lg[B:] ** 2)
        loss.backward()
        return float(loss.detach()), {n: t.grad.double().numpy() for n, t in sd.items()}

    # the torch side stepped alongside: its own parameters from the same start, its own AdamW, the native branch pattern
    sd_t = R.to_torch(sd_np, dtype=torch.float32, requires_grad=True)
    opt_t = torch.optim.AdamW(list(sd_t.values()), lr=1e-4)
    first = last = None
    for step in range(steps):
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        opt_n.zero_grad(set_to_none=True)
        ln, signs = 0, []
        for d in m.discriminators:
            logits, fmap, a0 = _captured_forward(d, x)
            signs.append(_native_signs(fmap, a0))
            ln = ln + torch.mean((1 - logits[:B]) ** 2) + torch.mean(logits[B:] ** 2)
        ln.backward()
        cpu = {n: t.cpu() for n, t in before.items()}
        lt, g32 = restated(cpu, signs, torch.float32)
        _, g64 = restated(cpu, signs, torch.float64)
        yards = _yardsticks(g32, g64)
        ratios = {n: R.rel_l2(_np(p.grad), g64[n]) / yards[n] for n, p in m.named_parameters()}
        worst = max(ratios, key=ratios.get)
        ln_ = float(ln.detach())
        rel = abs(ln_ - lt) / abs(lt)
        print(f"step {step}: native {ln_:.6f}  torch fp32 {lt:.6f}  relative difference {rel:.2e} (bar {lbar:.2e}); worst gradient {worst}: "
              f"{ratios[worst]:.2f} x torch fp32's distance from float64 (bar 4)")
        assert rel <= lbar, step
        assert ratios[worst] <= 4.0, (step, worst, ratios[worst])
        opt_t.zero_grad(set_to_none=True)
        la = 0
        for k, W in enumerate(R.FFT_SIZES):
            lg = R.forward(sd_t, xc, W, signs=signs[k], prefix=f"discriminators.{k}.").fmaps[-1]
            la = la + torch.mean((1 - lg[:B]) ** 2) + torch.mean(lg[B:] ** 2)
        la.backward()
        rel_a = abs(ln_ - float(la.detach())) / abs(float(la.detach()))
        print(f"        torch fp32 stepped alongside {float(la.detach()):.6f}  relative difference {rel_a:.2e} (bar 1e-3)")
        assert rel_a <= 1e-3, step
        opt_n.step()
        opt_t.step()
        assert all(not torch.equal(p.detach(), before[n]) for n, p in m.named_parameters())
        first, last = (ln_ if first is None else first), ln_
    assert last < first
    pn = np.concatenate([_np(p).reshape(-1) for _, p in m.named_parameters()])
    pt = np.concatenate([sd_t[n].detach().double().numpy().reshape(-1) for n, _ in m.named_parameters()])
    drift, moved = R.rel_l2(pn, pt), int((np.abs(pn - pt) > 1e-5).sum())
    print(f"parameters after {steps} steps against the side stepped alongside: relative L2 {drift:.2e} (bar 1e-4), {moved} of {pn.size} elements "
          f"apart by more than 1e-5")
    assert drift <= 1e-4
