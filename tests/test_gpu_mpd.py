"""The native multi-period discriminator (stabletts_amd/discriminator.py) on the GPU: forward and gradients against float64 --
the REAL reference module's (tests/golden/mpd_grads.npz) and, at shapes the fixture lacks, the torch restatement's
(tests/mpd_restatement.py, pinned to the real module by tests/test_mpd_cpu.py) -- determinism and independence, the module rules
and a short AdamW trajectory against torch autograd on the same GPU.

Metric: relative L2 distance per tensor over the stored elements (the fixture's rule).  Bars: 4 x the fixture's own
fp32-torch-vs-float64 error -- of that tensor where the fixture has it, else the largest the ``linear`` cases record -- both sides
being fp32 evaluations of the same function in another order.  Gradients in training mode are compared SIGN-CONSISTENTLY (see
mpd_restatement): the float64 side is evaluated at the branch pattern the native forward took, after asserting that this pattern
differs from float64's own only where the float64 value is within the forward bar of zero.  Every figure is printed beside its
bar.  Run with ``-m gpu``.
"""
import os

import numpy as np
import pytest
import torch

from tests import mpd_restatement as R
from tests import synth_weights as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu, pytest.mark.grad]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mpd_grads.npz")))


def _linear_bar(gold):
    return 4 * max(max(float(gold[c + "/err32"].max()), float(gold[c + "/dx_err32"].reshape(-1)[0])) for c in R.LINEAR_CASES)


def _fmap_bar(gold):
    return 4 * max(float(gold[c + "/fmap_err32"].max()) for c in list(R.LINEAR_CASES) + ["train_step"])


def _dp(period, sd_np, slope):
    from stabletts_amd.discriminator import DiscriminatorP
    d = DiscriminatorP(period, lrelu_slope=slope)
    d.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    return d.to("cuda:0").train()


def _mpd(sd_np):
    from stabletts_amd.discriminator import MultiPeriodDiscriminator
    m = MultiPeriodDiscriminator()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    return m.to("cuda:0").train()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _grads(mod):
    return {n: _np(p.grad) for n, p in mod.named_parameters()}


def _native_linear(d, x_np, wseed):
    d.zero_grad(set_to_none=True)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    logits, fmap = d(x)
    assert torch.equal(logits, torch.flatten(fmap[-1], 1, -1))
    R.linear_loss(fmap, wseed).backward()
    return [_np(f) for f in fmap], _grads(d), _np(x.grad)


_REF = {}


def _ref_linear(p, B, T, wseed, aseed):
    """float64 restatement on the CPU, computed once per shape."""
    key = (p, B, T, wseed, aseed)
    if key not in _REF:
        sd = R.to_torch(R.make_dp_state_dict(wseed), requires_grad=True)
        x = torch.from_numpy(R.make_audio(B, T, aseed)).double().requires_grad_(True)
        out = R.forward(sd, x, p, 1.0)
        R.linear_loss(out.fmaps, wseed).backward()
        _REF[key] = ([f.detach().numpy() for f in out.fmaps], {n: t.grad.numpy() for n, t in sd.items()}, x.grad.numpy())
    return _REF[key]


# ---- 1. forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.LINEAR_CASES))
def test_forward_linear_cases_against_the_real_module(gold, case):
    p, B, T, wseed, aseed = R.LINEAR_CASES[case]
    d = _dp(p, R.make_dp_state_dict(wseed), 1.0)
    with torch.no_grad():
        logits, fmap = d(torch.from_numpy(R.make_audio(B, T, aseed)).cuda())
    assert [",".join(map(str, f.shape)) for f in fmap] == gold[case + "/fmap_shapes"].tolist() and logits.shape == (B, fmap[-1][0].numel())
    for i, f in enumerate(fmap):
        err, bar = R.rel_l2(R.stored_elements(1000 + i, _np(f), wseed), gold[f"{case}/fmap/{i}"]), 4 * float(gold[case + "/fmap_err32"][i])
        print(f"{case} fmap {i}: {err:.2e} (bar {bar:.2e})")
        assert err <= bar, i


def test_forward_train_step_against_the_real_module(gold):
    seed = int(gold["train_step/seed"].reshape(-1)[0])
    B, T = R.TRAIN_STEP["B"], R.TRAIN_STEP["T"]
    m = _mpd(R.make_mpd_state_dict(seed))
    y, yh = torch.from_numpy(R.make_audio(B, T, seed + 1)).cuda(), torch.from_numpy(R.make_audio(B, T, seed + 2)).cuda()
    with torch.no_grad():
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = m(y, yh)
    for k in range(5):
        for i in range(5):
            f = torch.cat([fmap_rs[k][i], fmap_gs[k][i]])
            err = R.rel_l2(R.stored_elements(2000 + 10 * k + i, _np(f), seed), gold[f"train_step/fmap/{k}/{i}"])
            bar = 4 * float(gold["train_step/fmap_err32"][k][i])
            print(f"train_step period {R.PERIODS[k]} fmap {i}: {err:.2e} (bar {bar:.2e})")
            assert err <= bar, (k, i)
        err = R.rel_l2(_np(torch.cat([y_d_rs[k], y_d_gs[k]])), gold[f"train_step/logits/{k}"])
        bar = 4 * float(gold["train_step/fmap_err32"][k][4])
        print(f"train_step period {R.PERIODS[k]} logits: {err:.2e} (bar {bar:.2e})")
        assert err <= bar, k


# ---- 2. gradients, linear mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.LINEAR_CASES))
def test_gradients_linear_cases_against_the_real_module(gold, case):
    p, B, T, wseed, aseed = R.LINEAR_CASES[case]
    d = _dp(p, R.make_dp_state_dict(wseed), 1.0)
    _, grads, dx = _native_linear(d, R.make_audio(B, T, aseed), wseed)
    names = gold[case + "/names"].tolist()
    assert list(grads) == names
    fails = []
    for i, n in enumerate(names):
        err, own = R.rel_l2(R.stored_elements(i, grads[n], wseed), gold[f"{case}/grad/{n}"]), float(gold[case + "/err32"][i])
        print(f"{case} {n:48s} native {err:.2e}  torch fp32 {own:.2e}  ratio {err / own:5.2f} (bar 4)")
        if err > 4 * own:
            fails.append(n)
    err, own = R.rel_l2(dx, gold[case + "/dx64"]), float(gold[case + "/dx_err32"].reshape(-1)[0])
    print(f"{case} d x: native {err:.2e}  torch fp32 {own:.2e}  ratio {err / own:5.2f} (bar 4)")
    assert not fails and err <= 4 * own, fails


# (period, B, T): the smallest shapes at which the kernels can go wrong
SHAPES = [
    (11, 2, 12),        # n_pad = 10; H = 2 -> 1 at every layer
    (7, 2, 50),         # n_pad = 6
    (2, 2, 64), (3, 2, 99), (11, 2, 121),       # no pad
    (5, 2, 140), (5, 2, 145), (5, 2, 150),      # H = 28, 29, 30: the three residues of (H - 1) % 3 at the first strided layer
    (3, 3, 331),        # a ragged 32 / 64-frame tile in every layer, N no multiple of p x tile
    (7, 1, 50),         # a single item
    (2, 2, 4099),       # more than one split-K plane in the weight gradients
]


@pytest.mark.parametrize("p,B,T", SHAPES)
def test_gradients_linear_mode_at_the_edge_shapes(gold, p, B, T):
    """Slope 1.0 and the linear loss against the float64 restatement.  The last shape crosses the split-K plane of the weight
    gradient: at p = 2, B = 2, T = 4099 layers 1 and 2 see 912 and 304 frames, which wgrad_split cuts into 8 and 3 planes
    (asserted below on synth_weights' restatement of the rule); every smaller shape of the list runs one plane."""
    wseed, aseed = 400 + p, 500 + T
    if T == 4099:
        h = [(T + p - 1) // p]
        for s in R.STRIDES:
            h.append((h[-1] - 1) // s + 1)
        assert sw.wgrad_planes(B * h[2] * p, 32 * 5, 128) > 1 and sw.wgrad_planes(B * h[3] * p, 128 * 5, 512) > 1
    d = _dp(p, R.make_dp_state_dict(wseed), 1.0)
    fm, grads, dx = _native_linear(d, R.make_audio(B, T, aseed), wseed)
    rf, rg, rdx = _ref_linear(p, B, T, wseed, aseed)
    bar, fbar = _linear_bar(gold), _fmap_bar(gold)
    ferr = max(R.rel_l2(a, b) for a, b in zip(fm, rf))
    errs = {n: R.rel_l2(grads[n], rg[n]) for n in rg}
    worst = max(errs, key=errs.get)
    de = R.rel_l2(dx, rdx)
    print(f"p={p} B={B} T={T}: fmaps {ferr:.2e} (bar {fbar:.2e}), worst parameter {worst} {errs[worst]:.2e}, d x {de:.2e} (bar {bar:.2e})")
    assert [f.shape for f in fm] == [f.shape for f in rf]
    assert ferr <= fbar and de <= bar
    for n, e in errs.items():
        assert e <= bar, (n, e)


# ---- 3. gradients, training mode -------------------------------------------------------------------------------------------
def _torch_losses(y_d_rs, y_d_gs, fmap_rs, fmap_gs):
    """discriminator_loss + feature_loss + generator_loss (loss.py:37-66) on the returned tensors."""
    disc = sum(torch.mean((1 - dr) ** 2) + torch.mean(dg ** 2) for dr, dg in zip(y_d_rs, y_d_gs))
    feat = 2 * sum(torch.mean(torch.abs(rl - gl)) for dr, dg in zip(fmap_rs, fmap_gs) for rl, gl in zip(dr, dg))
    gen = sum(torch.mean((1 - dg) ** 2) for dg in y_d_gs)
    return disc + feat + gen


@pytest.mark.parametrize("case", ["train_step", "small"])
def test_gradients_training_mode_sign_consistent(gold, case):
    if case == "train_step":
        B, T, seed = R.TRAIN_STEP["B"], R.TRAIN_STEP["T"], int(gold["train_step/seed"].reshape(-1)[0])
    else:
        B, T, seed = R.TRAIN_SMALL["B"], R.TRAIN_SMALL["T"], R.TRAIN_SMALL["seed"]
    sd_np, y_np, yh_np = R.make_mpd_state_dict(seed), R.make_audio(B, T, seed + 1), R.make_audio(B, T, seed + 2)
    m = _mpd(sd_np)
    y, yh = torch.from_numpy(y_np).cuda(), torch.from_numpy(yh_np).cuda().requires_grad_(True)
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = m(y, yh)
    _torch_losses(y_d_rs, y_d_gs, fmap_rs, fmap_gs).backward()
    grads, dyh = _grads(m), _np(yh.grad)
    # float64 at its own signs: the forward reference, and the branch pattern to compare the native one with
    sd = R.to_torch(sd_np)
    y64, yh64 = torch.from_numpy(y_np).double(), torch.from_numpy(yh_np).double()
    with torch.no_grad():
        own = R.mpd_forward(sd, y64, yh64, 0.1)
        _, _, own_l1 = R.gan_losses(own, B)
    fbar = _fmap_bar(gold) if case == "small" else None
    signs, l1, flips = [], [], 0
    for k, o in enumerate(own):
        assert o.margin0 > 64 * 2.0 ** -24, (k, o.margin0)      # layer 0 is not returned: its signs are the restatement's own, and safe
        signs.append([None])
        l1.append([])
        for i in range(5):
            nat = torch.cat([fmap_rs[k][i], fmap_gs[k][i]]).detach().cpu().double()
            f64 = o.fmaps[i]
            fb = 4 * float(gold["train_step/fmap_err32"][k][i]) if fbar is None else fbar
            tol = fb * float(f64.norm())               # an element's error cannot exceed the tensor's L2 error
            assert R.rel_l2(nat.numpy(), f64.numpy()) <= fb
            if i < 4:                                  # leaky-ReLU branch of layers 1..4: the sign of the post-activation
                s = nat > 0
                diff = s != o.signs[i + 1]
                assert bool((f64[diff].abs() <= tol).all()), (k, i)
                flips += int(diff.sum())
                signs[-1].append(s)
            dn, d64 = nat[:B] - nat[B:], f64[:B] - f64[B:]
            s = dn > 0
            diff = s != own_l1[k][i]
            assert bool((d64[diff].abs() <= 2 * tol).all()), (k, i)
            flips += int(diff.sum())
            l1[-1].append(s)
    # float64 gradients at the native branch pattern
    sd = R.to_torch(sd_np, requires_grad=True)
    yh64 = yh64.requires_grad_(True)
    loss, _, _ = R.gan_losses(R.mpd_forward(sd, y64, yh64, 0.1, signs=signs), B, l1)
    loss.backward()
    bar = _linear_bar(gold)
    errs = {n: R.rel_l2(grads[n], sd[n].grad.numpy()) for n in sd}
    worst = max(errs, key=errs.get)
    de = R.rel_l2(dyh, yh64.grad.numpy())
    print(f"{case} (B={B}, T={T}): {flips} branch flips against float64's own signs; worst parameter {worst} {errs[worst]:.2e}, "
          f"d y_hat {de:.2e} (bar {bar:.2e})")
    if case == "train_step":
        real = {n: R.rel_l2(R.stored_elements(i, grads[n], seed), gold[f"train_step/grad/{n}"]) for i, n in enumerate(sd)}
        w2 = max(real, key=real.get)
        print(f"  distance to the real module's stored float64 gradients (its own signs): worst {w2} {real[w2]:.2e}, "
              f"d y_hat {R.rel_l2(dyh, gold['train_step/dyhat64']):.2e}")
    assert de <= bar
    for n, e in errs.items():
        assert e <= bar, (n, e)


# ---- 4. determinism and independence ---------------------------------------------------------------------------------------
def test_determinism_and_independence(gold):
    from stabletts_amd.discriminator import DiscriminatorP
    seed, B, T = 601, 3, 331
    sd_np, y_np, yh_np = R.make_mpd_state_dict(seed), R.make_audio(B, T, seed + 1), R.make_audio(B, T, seed + 2)
    m = _mpd(sd_np)

    def step():
        m.zero_grad(set_to_none=True)
        y, yh = torch.from_numpy(y_np).cuda(), torch.from_numpy(yh_np).cuda().requires_grad_(True)
        out = m(y, yh)
        _torch_losses(*out).backward()
        return out, {n: p.grad.clone() for n, p in m.named_parameters()}, yh.grad.clone()

    (a_rs, a_gs, a_fr, a_fg), ga, da = step()
    (b_rs, b_gs, b_fr, b_fg), gb, db = step()
    assert torch.equal(da, db) and all(torch.equal(ga[n], gb[n]) for n in ga)
    assert all(torch.equal(x, y) for fa, fb in ((a_fr, b_fr), (a_fg, b_fg)) for la, lb in zip(fa, fb) for x, y in zip(la, lb))
    # the halves of mpd(y, y_hat) are DiscriminatorP(y) and DiscriminatorP(y_hat) alone; an item alone is its rows of the batch
    with torch.no_grad():
        y, yh = torch.from_numpy(y_np).cuda(), torch.from_numpy(yh_np).cuda()
        for k, d in enumerate(m.discriminators):
            assert isinstance(d, DiscriminatorP)
            lr, fr = d(y)
            lg, fg = d(yh)
            assert torch.equal(lr, a_rs[k]) and torch.equal(lg, a_gs[k])
            assert all(torch.equal(u, v) for u, v in zip(fr, a_fr[k])) and all(torch.equal(u, v) for u, v in zip(fg, a_fg[k]))
            l1, f1 = d(y[1:2])
            assert torch.equal(l1, lr[1:2]) and all(torch.equal(u, v[1:2]) for u, v in zip(f1, fr))
    # batch parameter gradients = the sum of the items', within the bar (linear loss: the loss is a sum over the items)
    p, wseed = 3, 611
    d = _dp(p, R.make_dp_state_dict(wseed), 0.1)
    x_np = R.make_audio(B, T, 612)

    def lin(xs, rows):
        d.zero_grad(set_to_none=True)
        x = torch.from_numpy(xs).cuda()
        _, fmap = d(x)
        sum((f * torch.from_numpy(R.loss_weights((B,) + tuple(f.shape[1:]), wseed + 31 * i)[rows]).cuda()).sum() for i, f in enumerate(fmap)).backward()
        return _grads(d)

    whole = lin(x_np, slice(0, B))
    parts = [lin(x_np[b:b + 1], slice(b, b + 1)) for b in range(B)]
    bar = _linear_bar(gold)
    errs = {n: R.rel_l2(sum(q[n] for q in parts), whole[n]) for n in whole}
    worst = max(errs, key=errs.get)
    print(f"batch vs sum of items: worst {worst} {errs[worst]:.2e} (bar {bar:.2e})")
    assert errs[worst] <= bar


# ---- 5. module rules -------------------------------------------------------------------------------------------------------
def test_module_rules():
    from stabletts_amd import _lib
    from stabletts_amd.discriminator import DiscriminatorP
    seed, B, T = 701, 2, 97
    sd_np = R.make_mpd_state_dict(seed)
    m = _mpd(sd_np)
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

    # y_hat.detach(): parameter gradients only, bitwise those of the attached run
    fake = yh.clone().requires_grad_(True)
    attached = leg(m, fake)
    d_attached = fake.grad.clone()
    detached = leg(m, fake.detach())
    assert all(torch.equal(attached[n], detached[n]) for n in attached)
    # a frozen module: d y_hat bitwise that of the unfrozen run, no parameter gradient
    m.requires_grad_(False)
    fake2 = yh.clone().requires_grad_(True)
    frozen = leg(m, fake2)
    assert all(g is None for g in frozen.values()) and torch.equal(fake2.grad, d_attached)
    m.requires_grad_(True)
    # parameter hooks fire once each (what DDP installs); clip_grad_norm_ is finite
    fired = []
    hooks = [p.register_hook(lambda g, n=n: fired.append(n)) for n, p in m.named_parameters()]
    leg(m, yh)
    for h in hooks:
        h.remove()
    assert sorted(fired) == sorted(n for n, _ in m.named_parameters())
    assert all(p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all() for p in m.parameters())
    norm = torch.nn.utils.clip_grad_norm_(m.parameters(), 1000)
    assert torch.isfinite(norm) and norm > 0
    # a second backward through the same forward, and a backward after another forward, are refused
    d = m.discriminators[1]
    x = torch.cat([y, yh])
    logits, _ = d(x)
    logits.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="differentiated already"):
        logits.sum().backward()
    logits, _ = d(x)
    d(x)
    with pytest.raises(RuntimeError, match="activations are gone"):
        logits.sum().backward()
    # an SGD step changes the next forward, and the recomputed w follows g and v: a fresh module with the stepped state agrees bitwise
    with torch.no_grad():
        before, _ = d(x)
    opt = torch.optim.SGD(d.parameters(), lr=1e-2)
    d.zero_grad()
    logits, _ = d(x)
    logits.square().mean().backward()
    opt.step()
    with torch.no_grad():
        after, _ = d(x)
        fresh = DiscriminatorP(d.period).to("cuda:0")
        fresh.load_state_dict(d.state_dict(), strict=True)
        assert not torch.equal(after, before) and torch.equal(after, fresh(x)[0])
    logits, _ = d(x)
    opt.step()                                                   # a parameter update between forward and backward
    with pytest.raises(RuntimeError, match="activations are gone"):
        logits.sum().backward()
    # T <= n_pad raises (the reference's reflect pad raises there too); non-native configurations raise at construction
    d11 = m.discriminators[4]
    with pytest.raises(_lib.NativeError, match="too short"):
        d11(torch.zeros(1, 1, 5, device="cuda"))
    with torch.no_grad():
        assert d11(torch.zeros(1, 1, 6, device="cuda"))[0].shape == (1, 11)
    for bad in (dict(in_channels=2), dict(kernel_size=3), dict(stride=1)):
        with pytest.raises(NotImplementedError):
            DiscriminatorP(2, **bad)
    # the C ABI: bad sizes, null pointers, a backward that is not the held forward's, a handle of another kind
    eng, lib = d.engine(), _lib.load()
    import ctypes
    xs = x.contiguous()
    shapes = eng.period_disc_fmap_shapes(2 * B, T, d.period)
    fm = [torch.full(s, 7.0, device="cuda") for s in shapes]
    dx = torch.full((2 * B, 1, T), 7.0, device="cuda")
    gflat = torch.full((eng.grad_layout()[None],), 7.0, device="cuda")
    ptrs = (ctypes.c_void_p * 5)(*[f.data_ptr() for f in fm])
    holed = (ctypes.c_void_p * 5)(*[f.data_ptr() for f in fm[:4]], None)
    for fwd in (lib.st_period_disc_forward, lib.st_period_disc_train_forward):
        assert fwd(eng.handle, xs.data_ptr(), ptrs, 0, T, None) == _lib.ST_ERR_INVALID
        assert fwd(eng.handle, xs.data_ptr(), ptrs, 2 * B, 0, None) == _lib.ST_ERR_INVALID
        assert fwd(eng.handle, None, ptrs, 2 * B, T, None) == _lib.ST_ERR_INVALID
        assert fwd(eng.handle, xs.data_ptr(), None, 2 * B, T, None) == _lib.ST_ERR_INVALID
        assert fwd(eng.handle, xs.data_ptr(), holed, 2 * B, T, None) == _lib.ST_ERR_INVALID
        assert fwd(eng.handle, xs.data_ptr(), ptrs, 1 << 20, T, None) == _lib.ST_ERR_INVALID
    e11 = d11.engine()
    assert lib.st_period_disc_forward(e11.handle, xs.data_ptr(), ptrs, 1, 5, None) == _lib.ST_ERR_INVALID      # T <= n_pad
    assert lib.st_period_disc_train_backward(eng.handle, None, dx.data_ptr(), gflat.data_ptr(), 2 * B, T, None) == _lib.ST_ERR_INVALID
    eng.finalize()                                               # drops the held activations
    assert eng.train_serial() == 0
    assert lib.st_period_disc_train_backward(eng.handle, ptrs, dx.data_ptr(), gflat.data_ptr(), 2 * B, T, None) == _lib.ST_ERR_STATE
    assert b"st_period_disc_train_forward" in lib.st_last_error(eng.handle)
    assert lib.st_period_disc_train_forward(eng.handle, xs.data_ptr(), ptrs, 2 * B, T, None) == _lib.ST_OK
    assert eng.train_serial() > 0
    torch.cuda.synchronize()
    assert all(torch.isfinite(f).all() and not torch.all(f == 7.0) for f in fm)
    assert lib.st_period_disc_train_backward(eng.handle, ptrs, dx.data_ptr(), gflat.data_ptr(), 2 * B, T - 1, None) == _lib.ST_ERR_STATE
    assert lib.st_period_disc_train_backward(eng.handle, ptrs, dx.data_ptr(), gflat.data_ptr(), B, T, None) == _lib.ST_ERR_STATE
    dec = _lib.Engine(128, 256, 1024, 4, 6, 3, 256, "f16", 0)       # a handle of another kind
    assert lib.st_period_disc_train_forward(dec.handle, xs.data_ptr(), ptrs, 2 * B, T, None) == _lib.ST_ERR_STATE
    assert lib.st_period_disc_train_backward(dec.handle, ptrs, dx.data_ptr(), gflat.data_ptr(), 2 * B, T, None) == _lib.ST_ERR_STATE
    audio = torch.zeros(8, device="cuda")
    assert lib.st_vocos_train_forward(eng.handle, xs.data_ptr(), audio.data_ptr(), 1, 1, None) == _lib.ST_ERR_STATE
    dec.close()
    torch.cuda.synchronize()
    assert torch.all(dx == 7.0) and torch.all(gflat == 7.0)      # the error paths left the output buffers untouched


# ---- 6. trajectory ---------------------------------------------------------------------------------------------------------
def test_discriminator_leg_trajectory_against_torch_autograd():
    """Six AdamW steps of the discriminator leg (vocoders/vocos/train.py:74,98-110: lr 1e-4, mpd(y, y_hat.detach()),
    discriminator_loss) on the native module and on torch autograd of the restatement in fp32 on the same GPU."""
    seed, B, T, steps = 801, 2, 331, 6
    sd_np = R.make_mpd_state_dict(seed)
    y, yh = torch.from_numpy(R.make_audio(B, T, seed + 1)).cuda(), torch.from_numpy(R.make_audio(B, T, seed + 2)).cuda()
    m = _mpd(sd_np)
    opt_n = torch.optim.AdamW(m.parameters(), lr=1e-4)
    sd = R.to_torch(sd_np, dtype=torch.float32, device="cuda", requires_grad=True)
    opt_t = torch.optim.AdamW(list(sd.values()), lr=1e-4)
    worst, first, last = 0.0, None, None
    for i in range(steps):
        opt_n.zero_grad(set_to_none=True)
        y_d_rs, y_d_gs, _, _ = m(y, yh.detach())
        ln = sum(torch.mean((1 - dr) ** 2) + torch.mean(dg ** 2) for dr, dg in zip(y_d_rs, y_d_gs))
        ln.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1000)
        opt_n.step()
        opt_t.zero_grad(set_to_none=True)
        outs = R.mpd_forward(sd, y, yh, 0.1, margin=False)
        lt = 0
        for o in outs:
            lg = torch.flatten(o.fmaps[-1], 1, -1)
            lt = lt + torch.mean((1 - lg[:B]) ** 2) + torch.mean(lg[B:] ** 2)
        lt.backward()
        torch.nn.utils.clip_grad_norm_(list(sd.values()), 1000)
        opt_t.step()
        ln, lt = float(ln.detach()), float(lt.detach())
        rel = abs(ln - lt) / abs(lt)
        worst = max(worst, rel)
        first, last = (ln if first is None else first), ln
        print(f"step {i}: native {ln:.6f}  torch {lt:.6f}  relative difference {rel:.2e} (bar 1e-3)")
        assert rel <= 1e-3, i
    assert last < first
