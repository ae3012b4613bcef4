"""The native optimizer step (stabletts_amd.optim: AdamW, clip_grad_norm_; st_adamw_step / st_grad_norm / st_grad_clip) on a real
MI355X.  Run with ``-m gpu``.

Parity.  Truth is the float64 restatement (tests/optim_restatement.py, pinned to torch.optim.AdamW on float64 tensors by
tests/test_optim_cpu.py) from the same fp32 start and gradients; the yardstick is torch.optim.AdamW(foreach=False) in fp32 on the
same device.  An error is the max-abs difference over the concatenation of all tensors of a kind (p, exp_avg, exp_avg_sq) divided
by the max-abs of the truth, and the gate is e_native <= 4 x e_torch per kind: the project's margin for an fp32 kernel against
torch's fp32 (tests/test_gpu_mel_sweep.py).  The errors are taken over a whole list because the yardstick's own error on a
one-element tensor is often exactly zero; in the launch-boundary lists (tensors of 1 .. 300 elements) "every tensor passes the
gate" therefore means the gate over the list each tensor is in, and each tensor is ALSO bitwise what it is when stepped alone.

Bitwise.  The update is elementwise with explicitly rounded operations, so a tensor's new p, m, v are the same bits alone, at any
list position, on the 16-byte path and on the scalar path, whole or cut into views.  The norm is fp64 in one fixed order.

Measured on an MI355X (profiles/optim_parity.txt): see MEASURED below.
"""
import ctypes

import pytest
import torch

from tests import optim_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUP_A = dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1)
GROUP_B = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
KINDS = ("p", "exp_avg", "exp_avg_sq")

# MEASURED (MI355X, profiles/optim_parity.txt; ratio = e_native / e_torch_fp32 for p / exp_avg / exp_avg_sq, bar 4):
#   parity list, three steps   1.00 / 1.00 / 1.00 (1.31e-07 / 6.06e-08 / 7.42e-08 on both sides)
#   lists of M-1, M, M+1, 2M+3 1.00 / 1.00 / 1.00
#   2^24 + 7 elements          1.00 / 1.00 / 1.24 (exp_avg_sq 1.02e-07 vs torch 8.18e-08: the kernel evaluates v b2 + (1 - b2) g g as
#                              fma((1 - b2) g, g, round(v b2)), torch in its own order)
#   clip_grad_norm_            norm of the parity list 7.5e-10 from float64 (bar 2^-23 = 1.19e-07)


def _lib():
    from stabletts_amd import _lib
    return _lib.load()


def _cm():
    lib = _lib()
    return int(lib.st_optim_chunk()), int(lib.st_optim_max_tensors())


def _rand(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def _place(t, odd=False):
    """A CUDA copy of t: at a fresh allocation (16-byte aligned), or starting at element 1 of one (4-byte aligned only)."""
    if not odd:
        out = t.to(DEV).clone()
        assert out.numel() == 0 or out.data_ptr() % 16 == 0
        return out
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
    out = buf[1:]
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _leaf(t, odd=False):
    return _place(t, odd).detach().requires_grad_(True)


def parity_counts():
    C, _ = _cm()
    # (elements, parameter at an odd element, gradient at an odd element)
    return [(1, 0, 0), (3, 0, 0), (255, 0, 0), (C - 1, 0, 0), (C, 0, 0), (C + 1, 0, 0), (2 * C + 5, 0, 0), (0, 0, 0), (C + 3, 1, 0), (300, 0, 1)]


def _errors(got, want64):
    """max-abs over the concatenation / max-abs of the truth."""
    a = torch.cat([t.detach().double().cpu().reshape(-1) for t in got])
    b = torch.cat([t.detach().double().cpu().reshape(-1) for t in want64])
    return float((a - b).abs().max() / b.abs().max())


def _state_lists(opt, ps):
    return {"p": [p.detach() for p in ps], "exp_avg": [opt.state[p]["exp_avg"] for p in ps], "exp_avg_sq": [opt.state[p]["exp_avg_sq"] for p in ps]}


def _gate(name, e_native, e_torch):
    lines = []
    for k in KINDS:
        ratio = e_native[k] / e_torch[k] if e_torch[k] > 0 else (0.0 if e_native[k] == 0 else float("inf"))
        lines.append(f"{name}: {k:10s} native {e_native[k]:.3e}  torch fp32 {e_torch[k]:.3e}  ratio {ratio:5.2f} (bar 4)")
    print("\n".join(lines))
    for k in KINDS:
        assert e_native[k] <= 4 * e_torch[k], (name, k, e_native[k], e_torch[k])
    return lines


def parity_case():
    """The issue's parity list: three steps, two groups, one gradient missing at step 2 -> (e_native, e_torch, steps of the
    native optimizer's tensors)."""
    from stabletts_amd.optim import AdamW
    counts = parity_counts()
    start = [_rand(n, 100 + i) for i, (n, _, _) in enumerate(counts)]
    pn = [_leaf(t, odd=bool(po)) for t, (_, po, _) in zip(start, counts)]
    pt = [_leaf(t) for t in start]
    split = 5
    native = AdamW([dict(params=pn[:split], **GROUP_A), dict(params=pn[split:], **GROUP_B)])
    yard = torch.optim.AdamW([dict(params=pt[:split], **GROUP_A), dict(params=pt[split:], **GROUP_B)], foreach=False)
    truth = R.Adamw64(start)
    lag = 2
    for step in range(3):
        for i, (n, _, go) in enumerate(counts):
            if step == 1 and i == lag:
                pn[i].grad = pt[i].grad = None
                continue
            g = _rand(n, 1000 + 100 * step + i, scale=0.5 + i)
            pn[i].grad, pt[i].grad = _place(g, odd=bool(go)), _place(g)
            truth.step(i, g, **(GROUP_A if i < split else GROUP_B))
        assert native._native_device() == torch.device(DEV)           # the kernels, not the fallback
        native.step()
        yard.step()
    torch.cuda.synchronize()
    full = [i for i, (n, _, _) in enumerate(counts) if n > 0]
    want = {"p": truth.p, "exp_avg": truth.m, "exp_avg_sq": truth.v}
    sn, st = _state_lists(native, pn), _state_lists(yard, pt)
    e_native = {k: _errors([sn[k][i] for i in full], [want[k][i] for i in full]) for k in KINDS}
    e_torch = {k: _errors([st[k][i] for i in full], [want[k][i] for i in full]) for k in KINDS}
    return e_native, e_torch, [int(native.state[p]["step"]) for p in pn], truth.steps


def test_parity_three_steps_two_groups_against_float64():
    e_native, e_torch, steps, want_steps = parity_case()
    _gate("parity", e_native, e_torch)
    assert steps == want_steps and steps[2] == 2 and all(s == 3 for i, s in enumerate(steps) if i != 2)


# ---- one step of a list, natively, on the yardstick and in float64
def _step_native(values, grads, hyper, odd=None):
    """One native step of the list -> [(p, m, v)] as CPU tensors.  odd: indices placed 4 bytes past a 16-byte boundary."""
    from stabletts_amd.optim import AdamW
    odd = odd or ()
    ps = [_leaf(t, odd=i in odd) for i, t in enumerate(values)]
    for i, (p, g) in enumerate(zip(ps, grads)):
        p.grad = _place(g, odd=i in odd)
    opt = AdamW(ps, **hyper)
    assert opt._native_device() == torch.device(DEV)      # the kernels, not the fallback
    opt.step()
    torch.cuda.synchronize()
    return [(p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()) for p in ps]


def _step_torch(values, grads, hyper):
    ps = [_leaf(t) for t in values]
    for p, g in zip(ps, grads):
        p.grad = _place(g)
    opt = torch.optim.AdamW(ps, foreach=False, **hyper)
    opt.step()
    return [(p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()) for p in ps]


def _step_truth(values, grads, hyper):
    return [R.adamw_update(p, g, torch.zeros_like(p), torch.zeros_like(p), 1, hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"])
            for p, g in zip(values, grads)]


def _list_errors(got, truth):
    return {k: _errors([t[j] for t in got], [t[j] for t in truth]) for j, k in enumerate(KINDS)}


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def make_small_tensors():
    """2M + 3 tensors of 1 .. 300 elements with gradients, and each one's native step ALONE in a one-entry list."""
    _, M = _cm()
    n = 2 * M + 3
    sizes = torch.randint(1, 301, (n,), generator=torch.Generator().manual_seed(7)).tolist()
    sizes[0], sizes[1] = 1, 300
    values = [_rand(s, 2000 + i) for i, s in enumerate(sizes)]
    grads = [_rand(s, 5000 + i, scale=0.1 + (i % 5)) for i, s in enumerate(sizes)]
    alone = [_step_native([v], [g], GROUP_A)[0] for v, g in zip(values, grads)]
    return values, grads, alone


@pytest.fixture(scope="module")
def small_tensors():
    return make_small_tensors()


def boundary_case(small, length):
    values, grads, alone = small
    v, g = values[:length], grads[:length]
    got = _step_native(v, g, GROUP_A)
    truth = _step_truth(v, g, GROUP_A)
    return got, _list_errors(got, truth), _list_errors(_step_torch(v, g, GROUP_A), truth), alone[:length]


@pytest.mark.parametrize("which", ["M-1", "M", "M+1", "2M+3"])
def test_launch_boundary_lists(small_tensors, which):
    _, M = _cm()
    length = {"M-1": M - 1, "M": M, "M+1": M + 1, "2M+3": 2 * M + 3}[which]
    got, e_native, e_torch, alone = boundary_case(small_tensors, length)
    _gate(f"list of {which} = {length}", e_native, e_torch)
    for i, (a, b) in enumerate(zip(got, alone)):
        assert _same_bits(a, b), f"tensor {i} of {length} differs from its step alone"


def test_bitwise_alone_any_position_either_path_and_repeatable(small_tensors):
    C, M = _cm()
    values, grads, _ = small_tensors
    for n in (C + 1, 2 * C + 5):
        v, g = _rand(n, 31 + n), _rand(n, 32 + n, scale=3.0)
        alone = _step_native([v], [g], GROUP_A)[0]
        assert _same_bits(alone, _step_native([v], [g], GROUP_A)[0])                       # two runs
        assert _same_bits(alone, _step_native([v], [g], GROUP_A, odd=(0,))[0])             # 4 bytes past a 16-byte boundary: scalar path
        assert not torch.equal(alone[0], v) and float(alone[2].abs().max()) > 0
        others_v, others_g = values[:M + 2], grads[:M + 2]
        for pos in (0, 1, M - 1, M, M + 2):                                                # first, inside, across the launch boundary, last
            lv, lg = others_v[:pos] + [v] + others_v[pos:], others_g[:pos] + [g] + others_g[pos:]
            assert _same_bits(alone, _step_native(lv, lg, GROUP_A)[pos]), (n, pos)
            assert _same_bits(alone, _step_native(lv, lg, GROUP_A, odd=(pos,))[pos]), (n, pos)


def test_many_chunks_one_tensor_and_its_two_views():
    from stabletts_amd.optim import AdamW
    C, _ = _cm()
    n = 2 ** 24 + 7
    gen = torch.Generator(device=DEV).manual_seed(5)
    v0 = torch.randn(n, device=DEV, generator=gen)
    g0 = torch.randn(n, device=DEV, generator=gen) * 2.0

    def run(cls, cut=None, **kw):
        flat = v0.clone()
        gflat = g0.clone()
        ps = [flat] if cut is None else [flat[:cut], flat[cut:]]
        gs = [gflat] if cut is None else [gflat[:cut], gflat[cut:]]
        ps = [p.detach().requires_grad_(True) for p in ps]
        for p, g in zip(ps, gs):
            p.grad = g
        opt = cls(ps, **GROUP_A, **kw)
        assert cls is not AdamW or opt._native_device() == torch.device(DEV)
        opt.step()
        return tuple(torch.cat([x.reshape(-1) for x in col]) for col in
                     ([p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps]))

    whole = run(AdamW)
    yard = run(torch.optim.AdamW, foreach=False)
    truth = R.adamw_update(v0, g0, torch.zeros_like(v0), torch.zeros_like(v0), 1, **GROUP_A)
    err = lambda got: {k: float((got[j].double() - truth[j]).abs().max() / truth[j].abs().max()) for j, k in enumerate(KINDS)}      # noqa: E731
    _gate("2^24 + 7 elements", err(whole), err(yard))
    views = run(AdamW, cut=C * 1000)                      # the same data as two views: the update is elementwise
    assert all(torch.equal(a, b) for a, b in zip(whole, views))
    views = run(AdamW, cut=C * 1000 + 1)                  # ... the second one on the scalar path
    assert all(torch.equal(a, b) for a, b in zip(whole, views))


def test_fallbacks_are_torch_adamw_bitwise():
    from stabletts_amd.optim import AdamW
    cases = {"amsgrad": (torch.float32, dict(amsgrad=True), False), "fp16": (torch.float16, {}, False),
             "non-contiguous gradient": (torch.float32, {}, True)}
    for name, (dtype, kw, strided) in cases.items():
        outs = []
        for cls in (AdamW, torch.optim.AdamW):
            ps = [_rand(24, 1).reshape(4, 6).to(DEV, dtype).requires_grad_(True), _rand(5, 2).to(DEV, dtype).requires_grad_(True)]
            opt = cls(ps, **GROUP_A, **kw)
            for step in range(2):
                g0 = _rand(24, 10 + step).to(DEV, dtype)
                ps[0].grad = g0.reshape(6, 4).t() if strided else g0.reshape(4, 6)
                ps[1].grad = _rand(5, 20 + step).to(DEV, dtype)
                assert ps[0].grad.is_contiguous() != strided
                assert cls is not AdamW or opt._native_device() is None
                opt.step()
            outs.append([t.cpu() for p in ps for t in [p.detach()] + [opt.state[p][k] for k in sorted(opt.state[p])]])
        assert len(outs[0]) == len(outs[1]) and all(torch.equal(a, b) for a, b in zip(*outs)), name


def test_version_counters_grow_for_updated_parameters_only():
    from stabletts_amd.optim import AdamW
    ps = [_leaf(_rand(n, 40 + n), odd=odd) for n, odd in ((5, False), (300, True), (9000, False))]
    for p in ps[:2]:
        p.grad = torch.ones_like(p)
    before = [p._version for p in ps]
    opt = AdamW(ps, **GROUP_A)
    opt.step()
    after = [p._version for p in ps]
    assert after[0] > before[0] and after[1] > before[1] and after[2] == before[2]
    assert ps[2] not in opt.state or not opt.state[ps[2]]
    with torch.inference_mode():                          # an inference tensor has no counter to bump: the step itself still runs
        q = torch.ones(7, device=DEV)
        q.grad = torch.ones(7, device=DEV)
        AdamW([q], **GROUP_A).step()
        assert float(q.max()) < 1.0


def test_native_state_is_torchs_state():
    """After native steps ``state`` holds what torch's optimizer holds: ``step`` a 0-dim CPU fp32 tensor with the count, the
    moments fp32 on the device; the state dict loads into torch.optim.AdamW, which continues from it, and back."""
    import copy

    from stabletts_amd.optim import AdamW
    vals = [_rand(n, 60 + n) for n in (5, 300, 9000)]
    ps = [_leaf(v) for v in vals]
    opt = AdamW([dict(params=ps[:2], **GROUP_A), dict(params=ps[2:], **GROUP_B)])
    for step in range(2):
        for i, p in enumerate(ps):
            p.grad = None if (step, i) == (1, 1) else _place(_rand(p.numel(), 70 + 10 * step + i))
        opt.step()
    assert [float(opt.state[p]["step"]) for p in ps] == [2.0, 1.0, 2.0]
    for p in ps:
        st = opt.state[p]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"]
        assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and st["step"].dim() == 0
        assert st["exp_avg"].device == p.device and st["exp_avg"].shape == p.shape
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    other = torch.optim.AdamW([dict(params=qs[:2], **GROUP_A), dict(params=qs[2:], **GROUP_B)], foreach=False)
    other.load_state_dict(copy.deepcopy(opt.state_dict()))
    back = AdamW([dict(params=[q.detach().clone().requires_grad_(True) for q in qs[:2]], **GROUP_A),
                  dict(params=[qs[2].detach().clone().requires_grad_(True)], **GROUP_B)])
    back.load_state_dict(copy.deepcopy(other.state_dict()))
    rs = [p for g in back.param_groups for p in g["params"]]
    for p, q, r in zip(ps, qs, rs):
        p.grad = _place(_rand(p.numel(), 99))
        q.grad, r.grad = p.grad.clone(), p.grad.clone()
    opt.step()
    other.step()
    back.step()
    assert [float(other.state[q]["step"]) for q in qs] == [3.0, 2.0, 3.0] == [float(back.state[r]["step"]) for r in rs]
    for p, q, r in zip(ps, qs, rs):
        assert torch.equal(p.detach(), r.detach()) and all(torch.equal(opt.state[p][k], back.state[r][k]) for k in ("exp_avg", "exp_avg_sq"))
        assert torch.allclose(p.detach(), q.detach(), rtol=1e-5, atol=1e-7)       # torch continues from the native state


@pytest.mark.grad
def test_native_module_sees_the_native_step():
    """Forward, backward, a native AdamW.step(), forward again on the smallest native Vocos generator of the suite: the inference
    path packs 16-bit weight copies and re-packs them when a version counter moves, so without the bump after the raw-pointer
    update the second forward would repeat the first."""
    import types

    from oracle import vocos_oracle as vo
    from stabletts_amd.optim import AdamW
    from stabletts_amd.vocos_train import Vocos
    cfg = vo.vocos_config(input_channels=64, intermediate_dim=256, num_layers=2)
    cfgs = (types.SimpleNamespace(input_channels=cfg.input_channels, dim=cfg.dim, intermediate_dim=cfg.intermediate_dim, num_layers=cfg.num_layers),
            types.SimpleNamespace(n_fft=cfg.n_fft, hop_length=cfg.hop_length))
    mod = Vocos(*cfgs)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in vo.make_vocos_state_dict(21, cfg).items()}, strict=True)
    mod = mod.to(DEV).train()
    mel = torch.from_numpy(vo.make_mel(2, 7, 22, M=cfg.input_channels)).to(DEV)
    with torch.no_grad():
        first = mod(mel).clone()
    opt = AdamW(mod.parameters(), lr=1e-2)
    audio = mod(mel)
    assert audio.requires_grad
    (audio * torch.randn(audio.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))).sum().backward()
    versions = [p._version for p in mod.parameters()]
    assert opt._native_device() == torch.device(DEV)
    opt.step()
    assert all(p._version > v for p, v in zip(mod.parameters(), versions))
    with torch.no_grad():
        second = mod(mel).clone()
    assert torch.isfinite(second).all() and not torch.equal(first, second)
    fresh = Vocos(*cfgs)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}, strict=True)
    fresh = fresh.to(DEV).train()
    with torch.no_grad():
        assert torch.equal(fresh(mel), second)
    assert torch.equal(fresh(mel).detach(), mod(mel).detach())          # and the training forward reads the updated fp32 weights


# ---- clip_grad_norm_
def _grad_list(seed=0, scale=1.0):
    """Parameters with gradients of the parity counts (one misaligned, one zero-element, one without a gradient)."""
    ps = []
    for i, (n, po, go) in enumerate(parity_counts()):
        p = _leaf(torch.zeros(n))
        p.grad = _place(_rand(n, 300 + 17 * seed + i, scale=scale), odd=bool(po or go))
        ps.append(p)
    ps.append(_leaf(torch.zeros(11)))                     # grad is None
    return ps


def _grads(ps):
    return [p.grad.detach().clone() for p in ps if p.grad is not None]


def test_clip_norm_below_max_norm_leaves_the_gradients_untouched():
    from stabletts_amd.optim import clip_grad_norm_
    ps = _grad_list()
    before = _grads(ps)
    want = R.total_norm(before)
    norm = clip_grad_norm_(ps, 1000.0)
    assert isinstance(norm, torch.Tensor) and norm.dim() == 0 and norm.dtype == torch.float32 and norm.device == torch.device(DEV)
    print(f"norm {float(norm):.9g} vs float64 {want:.9g}: rel {abs(float(norm) - want) / want:.2e} (bar 2^-23 = {2.0 ** -23:.2e})")
    assert abs(float(norm) - want) <= 2.0 ** -23 * want
    assert all(torch.equal(a, b) for a, b in zip(before, _grads(ps)))
    assert torch.equal(norm, clip_grad_norm_(ps, 1000.0))                                   # two runs
    assert torch.equal(norm, clip_grad_norm_(iter(ps), want * 1.001, norm_type=2, foreach=True))
    assert float(clip_grad_norm_([ps[-1]], 1.0)) == 0.0 and float(clip_grad_norm_([], 1.0)) == 0.0


def test_clip_norm_above_max_norm_scales_by_the_fp32_coefficient():
    from stabletts_amd.optim import clip_grad_norm_
    for max_norm in (1.0, 37.5):
        ps = _grad_list(seed=1, scale=2.0)
        before = _grads(ps)
        want = R.total_norm(before)
        assert want > max_norm
        norm = clip_grad_norm_(ps, max_norm)
        assert abs(float(norm) - want) <= 2.0 ** -23 * want
        coef = R.clip_coef(norm, max_norm).to(DEV)
        assert float(coef) < 1.0
        for a, b in zip(before, _grads(ps)):
            assert torch.equal(a * coef, b)
        after = R.total_norm(_grads(ps))
        assert abs(after - max_norm) <= 1e-5 * max_norm


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_clip_nonfinite_gradients_behave_as_in_torch(bad):
    from stabletts_amd.optim import clip_grad_norm_
    ps, pt = _grad_list(seed=2), _grad_list(seed=2)
    for lst in (ps, pt):
        lst[5].grad[17] = bad
    norm, want = clip_grad_norm_(ps, 2.0), torch.nn.utils.clip_grad_norm_(pt, 2.0)
    assert torch.equal(torch.isnan(norm), torch.isnan(want)) and (torch.isnan(want) or torch.equal(norm, want))
    assert torch.isnan(norm) if bad != bad else torch.isinf(norm)
    for a, b in zip(_grads(ps), _grads(pt)):
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
        if bad != bad:
            assert torch.isnan(a).all()
    if bad == bad:
        g = ps[5].grad
        assert torch.isnan(g[17]) and int(torch.isnan(g).sum()) == 1 and float(g.nan_to_num(nan=0.0).abs().max()) == 0.0


def test_clip_long_lists_concatenation_and_addresses(small_tensors):
    from stabletts_amd.optim import clip_grad_norm_
    _, M = _cm()
    values, _, _ = small_tensors

    def params(length, odd=()):
        ps = [_leaf(torch.zeros(v.numel())) for v in values[:length]]
        for i, (p, v) in enumerate(zip(ps, values)):
            p.grad = _place(v, odd=i in odd)
        return ps

    for length in (M + 1, 2 * M + 3):
        ps = params(length)
        want = R.total_norm(values[:length])
        norm = clip_grad_norm_(ps, 1e9)
        assert abs(float(norm) - want) <= 2.0 ** -23 * want, length
        cat = _leaf(torch.zeros(sum(v.numel() for v in values[:length])))
        cat.grad = torch.cat([p.grad for p in ps])
        assert abs(float(clip_grad_norm_([cat], 1e9)) - float(norm)) <= 2.0 ** -23 * want, length
        assert torch.equal(norm, clip_grad_norm_(params(length), 1e9))                      # two runs
        assert torch.equal(norm, clip_grad_norm_(params(length, odd=(0, 1, M, length - 1)), 1e9))      # an entry's address does not matter
        # clipped: every gradient of a long list by the one coefficient
        norm = clip_grad_norm_(ps, 0.5)
        coef = R.clip_coef(norm, 0.5).to(DEV)
        for p, v in zip(ps, values):
            assert torch.equal(p.grad, v.to(DEV) * coef)
    C, _ = _cm()
    big = _rand(2 * C + 5, 77)
    one, other = _leaf(torch.zeros(big.numel())), _leaf(torch.zeros(big.numel()))
    one.grad, other.grad = _place(big), _place(big, odd=True)
    assert torch.equal(clip_grad_norm_([one], 1e9), clip_grad_norm_([other], 1e9))


def test_c_abi_norm_of_an_empty_list_is_zero():
    lib = _lib()
    out = torch.full((1,), 3.0, device=DEV)
    with torch.cuda.device(DEV):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.st_grad_norm(None, None, 0, out.data_ptr(), None, 0, stream) == 0
    assert float(out) == 0.0
