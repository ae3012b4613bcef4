"""CPU checks of the native optimizer step (stabletts_amd/optim.py): on CPU tensors the drop-in is torch's optimizer bit for bit,
its state dict is torch's, the C entry points check their arguments before anything touches a device, and the float64
restatement the GPU tests use as truth (tests/optim_restatement.py) is torch.optim.AdamW on float64 tensors."""
import copy
import ctypes

import pytest
import torch

from tests import optim_restatement as R

SHAPES = [(7,), (3, 5), (1,), (2, 3, 4)]


def _params(seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g, dtype=dtype).requires_grad_(True) for s in SHAPES]


def _groups(ps):
    return [dict(params=ps[:2], lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1),
            dict(params=ps[2:3], lr=1e-2, weight_decay=0.0),
            dict(params=ps[3:], lr=2e-3, amsgrad=True)]


def _set_grads(ps, seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(ps):
        grad = torch.randn(p.shape, generator=g, dtype=p.dtype)
        p.grad = None if i in skip else grad


def _same_state(a, b, pa, pb):
    for x, y in zip(pa, pb):
        assert torch.equal(x.detach(), y.detach())
        sa, sb = a.state.get(x, {}), b.state.get(y, {})
        assert sorted(sa) == sorted(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and sa[k].device == sb[k].device and torch.equal(sa[k], sb[k]), k


def test_cpu_parameters_step_bitwise_as_torch_adamw():
    from stabletts_amd.optim import AdamW
    pa, pb = _params(1), _params(1)
    a, b = AdamW(_groups(pa)), torch.optim.AdamW(_groups(pb))
    assert isinstance(a, torch.optim.AdamW)
    calls = []
    a.register_step_post_hook(lambda *_: calls.append(1))
    for step in range(5):
        skip = (1,) if step == 2 else ()                  # a parameter without a gradient is skipped: no state, no step counted
        _set_grads(pa, 10 + step, skip)
        _set_grads(pb, 10 + step, skip)
        a.step()
        b.step()
        _same_state(a, b, pa, pb)
    assert len(calls) == 5                                # the step hooks run once per step on the fallback too
    assert float(a.state[pa[0]]["step"]) == 5 and float(a.state[pa[1]]["step"]) == 4
    assert "max_exp_avg_sq" in a.state[pa[3]]

    # a closure is evaluated with gradients enabled and its loss returned, as in the parent
    def closure_of(ps, opt):
        def closure():
            opt.zero_grad()
            loss = sum((p ** 2).sum() for p in ps)
            loss.backward()
            return loss
        return closure
    la, lb = a.step(closure_of(pa, a)), b.step(closure_of(pb, b))
    assert torch.equal(la, lb)
    _same_state(a, b, pa, pb)


def test_clip_grad_norm_on_cpu_is_torchs_function():
    from stabletts_amd.optim import clip_grad_norm_
    for kw in (dict(norm_type=float("inf")), dict(norm_type=2.0), dict(norm_type=2.0, error_if_nonfinite=True), dict(norm_type=1.0, foreach=False)):
        pa, pb = _params(2), _params(2)
        _set_grads(pa, 3, skip=(2,))
        _set_grads(pb, 3, skip=(2,))
        na, nb = clip_grad_norm_(pa, 0.5, **kw), torch.nn.utils.clip_grad_norm_(pb, 0.5, **kw)
        assert na.dtype == nb.dtype and na.shape == nb.shape and torch.equal(na, nb)
        for x, y in zip(pa, pb):
            assert (x.grad is None and y.grad is None) or torch.equal(x.grad, y.grad)
    pa = _params(2)
    _set_grads(pa, 3)
    pa[0].grad[0] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(pa, 0.5, error_if_nonfinite=True)
    with pytest.raises(RuntimeError, match="non-finite"):
        torch.nn.utils.clip_grad_norm_(pa, 0.5, error_if_nonfinite=True)
    # an empty list, a single tensor, a generator
    out = clip_grad_norm_([], 1.0)
    assert torch.equal(out, torch.nn.utils.clip_grad_norm_([], 1.0)) and out.dtype == torch.float32 and out.dim() == 0
    pb = _params(2)
    _set_grads(pb, 3)
    assert torch.equal(clip_grad_norm_(pa[1], 1.0, norm_type=float("inf")), torch.nn.utils.clip_grad_norm_(pb[1], 1.0, norm_type=float("inf")))
    assert torch.equal(pa[1].grad, pb[1].grad)
    pb = _params(2)
    _set_grads(pb, 4)
    want = torch.nn.utils.clip_grad_norm_([p.detach().clone().requires_grad_(True) for p in pb], 1e9)      # no gradients: tensor(0.)
    assert float(want) == 0.0
    assert float(clip_grad_norm_((p for p in pb), 1e9)) == pytest.approx(R.total_norm([p.grad for p in pb]), rel=1e-6)


def test_state_dict_round_trip_between_the_two_classes():
    from stabletts_amd.optim import AdamW
    pa, pb = _params(5), _params(5)
    a, b = AdamW(_groups(pa)[:2]), torch.optim.AdamW(_groups(pb)[:2])
    for step in range(2):
        _set_grads(pa, 20 + step)
        a.step()
    sd = a.state_dict()
    assert sd["param_groups"] == torch.optim.AdamW(_groups(_params(5))[:2]).state_dict()["param_groups"]
    b.load_state_dict(copy.deepcopy(sd))                  # load_state_dict keeps same-dtype tensors by reference
    sb = b.state_dict()
    assert sb["param_groups"] == sd["param_groups"] and sorted(sb["state"]) == sorted(sd["state"])
    for k, st in sd["state"].items():
        assert sorted(st) == sorted(sb["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        for name in st:
            assert torch.equal(st[name], sb["state"][k][name])
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 2
    c = AdamW(_groups(_params(5))[:2])
    c.load_state_dict(copy.deepcopy(sb))                  # and back
    sc = c.state_dict()
    for k, st in sd["state"].items():
        assert all(torch.equal(st[name], sc["state"][k][name]) for name in st)
        assert sc["state"][k]["step"].device.type == "cpu" and sc["state"][k]["step"].dtype == torch.float32
    # the two continue identically from the loaded state
    with torch.no_grad():
        for x, y in zip(pb, pa):
            x.copy_(y)
    _set_grads(pa, 30)
    _set_grads(pb, 30)
    a.step()
    b.step()
    _same_state(a, b, pa[:3], pb[:3])
    sched = torch.optim.lr_scheduler.ExponentialLR(a, gamma=0.5)       # torch's schedulers take the class as it is
    a.step()
    sched.step()
    assert a.param_groups[0]["lr"] == pytest.approx(1.5e-3)


def test_restatement_is_torch_adamw_on_float64():
    ps = _params(7, torch.float64)
    groups = _groups(ps)[:2]
    opt = torch.optim.AdamW(groups, foreach=False)
    ref = R.Adamw64(ps[:3])
    for step in range(3):
        _set_grads(ps, 40 + step, skip=(1,) if step == 1 else ())
        for gi, group in enumerate(groups):
            for p in group["params"]:
                i = next(k for k, q in enumerate(ps) if q is p)
                if p.grad is not None:
                    ref.step(i, p.grad, group["lr"], group.get("betas", (0.9, 0.999)), group.get("eps", 1e-8), group["weight_decay"])
        opt.step()
        for i in range(3):
            st = opt.state[ps[i]]
            for got, want in ((ref.p[i], ps[i].detach()), (ref.m[i], st["exp_avg"]), (ref.v[i], st["exp_avg_sq"])):
                assert float((got - want).abs().max() / want.abs().max()) <= 1e-15
            assert ref.steps[i] == int(st["step"])
    assert ref.steps == [3, 2, 3]
    g = [torch.tensor([3.0, 0.0]), torch.tensor([[4.0]])]
    assert R.total_norm(g) == 5.0
    assert float(R.clip_coef(torch.tensor(5.0), 1000.0)) == 1.0 and float(R.clip_coef(torch.tensor(5.0), 2.5)) == pytest.approx(0.5, rel=1e-6)


def test_abi_symbols_and_host_side_argument_checks():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    lib = _lib.load()
    for name in ("st_optim_chunk", "st_optim_max_tensors", "st_grad_norm_scratch_bytes", "st_grad_norm", "st_grad_clip", "st_adamw_step"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    C, M = lib.st_optim_chunk(), lib.st_optim_max_tensors()
    # the widest table entry: four pointers, a 64-bit count, the first block, two floats (padded to 8 bytes) = 56 bytes
    assert C >= 1024 and C % 1024 == 0 and M >= 2 and M * 56 <= 4096
    INV = _lib.ST_ERR_INVALID
    i64s = lambda *v: (ctypes.c_int64 * len(v))(*v)       # noqa: E731
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)      # noqa: E731
    err = lambda: lib.st_last_error(None).decode()        # noqa: E731

    # scratch: one fp64 partial per chunk, monotone in the list
    assert lib.st_grad_norm_scratch_bytes(None, 0) == 0
    assert lib.st_grad_norm_scratch_bytes(i64s(1), 1) == 8
    sizes = [1, C - 1, C, C + 1, 3 * C + 5]
    got = [lib.st_grad_norm_scratch_bytes(i64s(*sizes[:k]), k) for k in range(len(sizes) + 1)]
    assert got == [0, 8, 16, 24, 40, 72] and got == sorted(got)
    assert lib.st_grad_norm_scratch_bytes(i64s(C), 1) <= lib.st_grad_norm_scratch_bytes(i64s(C + 1), 1)
    assert lib.st_grad_norm_scratch_bytes(None, 1) == INV and lib.st_grad_norm_scratch_bytes(i64s(4), -1) == INV
    assert lib.st_grad_norm_scratch_bytes(i64s(4, 0), 2) == INV and err() == "every element count must be >= 1"

    # fake but well-formed device addresses: every call below must return before anything is launched
    a, b, c, d, out, scr = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    n1, s1 = i64s(10), i64s(1)
    ok = dict(norm=(ptrs(a), n1, 1, out, scr, 8, None), clip=(ptrs(a), n1, 1, out, 1.0, None),
              adamw=(ptrs(a), ptrs(b), ptrs(c), ptrs(d), n1, s1, 1, 1e-3, 0.9, 0.999, 1e-8, 1e-2, None))
    fns = dict(norm=lib.st_grad_norm, clip=lib.st_grad_clip, adamw=lib.st_adamw_step)
    idx = dict(norm=dict(grads=0, numels=1, n=2, out=3, scratch=4, nbytes=5), clip=dict(grads=0, numels=1, n=2, norm=3),
               adamw=dict(params=0, grads=1, m=2, v=3, numels=4, steps=5, n=6))

    def bad(kind, **over):
        args = list(ok[kind])
        for k, v in over.items():
            args[idx[kind][k]] = v
        rc = fns[kind](*args)
        assert rc != INV or err(), (kind, over)            # every refusal says why
        return rc

    for kind, arrays in (("norm", ["grads"]), ("clip", ["grads"]), ("adamw", ["params", "grads", "m", "v"])):
        for name in arrays:
            assert bad(kind, **{name: None}) == INV, (kind, name)                     # null array
            assert bad(kind, **{name: ptrs(None)}) == INV and err() == "null tensor pointer", (kind, name)
            assert bad(kind, **{name: ptrs(a + 2)}) == INV, (kind, name)              # not 4-byte aligned
            assert bad(kind, **{name: ptrs(a + 1)}) == INV and err() == "tensor pointers must be 4-byte aligned", (kind, name)
        assert bad(kind, numels=None) == INV and bad(kind, n=-1) == INV, kind
        assert bad(kind, numels=i64s(0)) == INV and bad(kind, numels=i64s(-3)) == INV, kind
    assert bad("norm", out=None) == INV and bad("norm", scratch=None) == INV and bad("norm", out=out + 2) == INV
    assert bad("norm", nbytes=7) == INV and err() == "scratch is smaller than st_grad_norm_scratch_bytes() of this list"
    assert bad("norm", numels=i64s(C + 1), nbytes=8) == INV                           # two chunks need 16 bytes
    assert bad("norm", scratch=scr + 4) == INV
    assert bad("clip", norm=None) == INV and bad("clip", norm=out + 1) == INV
    assert bad("adamw", steps=None) == INV and bad("adamw", steps=i64s(0)) == INV and bad("adamw", steps=i64s(-2)) == INV
    assert "step" in err()
    # a bad entry beyond the first launch group is found before the first group is launched
    n = M + 2
    many = ptrs(*([a] * n))
    assert lib.st_adamw_step(many, many, many, many, i64s(*([4] * n)), i64s(*([1] * (n - 1) + [0])), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, None) == INV
    assert lib.st_grad_clip(ptrs(*([a] * (n - 1) + [a + 2])), i64s(*([4] * n)), n, out, 1.0, None) == INV
    assert lib.st_grad_norm(many, i64s(*([4] * (n - 1) + [0])), n, out, scr, 8 * n, None) == INV
