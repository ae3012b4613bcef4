"""The optimizer step of both training loops on native gfx950 kernels: ``AdamW`` and ``clip_grad_norm_`` with the signatures of
``torch.optim.AdamW`` and ``torch.nn.utils.clip_grad_norm_``.

    from stabletts_amd.optim import AdamW, clip_grad_norm_

``AdamW`` IS a ``torch.optim.AdamW``: ``param_groups``, ``state`` (``step`` a CPU fp32 tensor, ``exp_avg``, ``exp_avg_sq``),
``state_dict()`` / ``load_state_dict()``, ``zero_grad()`` and the LR schedulers are torch's own, and a checkpoint of either class
loads into the other.  Only ``step()`` differs: one multi-tensor launch per 64 parameters of a group (``st_adamw_step``, the table
of pointers a kernel argument) instead of the foreach optimizer's chain of launches, each element updated by explicitly rounded
fp32 operations whose result does not depend on the list, the address or the launch.  After the launches every updated
parameter's version counter is bumped, which is how the native modules learn that their packed weights are stale.

The native path runs when every parameter of the step that has a gradient is a dense, contiguous CUDA fp32 tensor on one device
with a contiguous fp32 gradient and contiguous states, and ``amsgrad``, ``maximize``, ``capturable``, ``differentiable`` and
``fused`` are off in every group.  Anything else -- CPU tensors, other dtypes, a non-contiguous gradient -- is the whole step by
``torch.optim.AdamW.step``, so the class works everywhere.

``clip_grad_norm_`` computes the 2-norm with fp64 accumulation in one fixed order (``st_grad_norm``) and scales the gradients by a
coefficient formed on the device (``st_grad_clip``; no host synchronisation, and no second pass when nothing is clipped).  Other
norm types, ``error_if_nonfinite=True`` and gradients that are not contiguous CUDA fp32 on one device go to torch's function.
"""
import ctypes

import torch

from . import _lib

__all__ = ["AdamW", "clip_grad_norm_"]


def _check(rc):
    if rc != _lib.ST_OK:
        raise _lib.NativeError(rc, _lib.load().st_last_error(None).decode())


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _counts(tensors):
    return (ctypes.c_int64 * len(tensors))(*[t.numel() for t in tensors])


def _dense_f32(t, idx):
    """t is a dense, contiguous fp32 tensor on CUDA device idx (attribute reads only: this runs per tensor and step)."""
    return (t.dtype is torch.float32 and t.is_cuda and t.get_device() == idx and t.layout is torch.strided and t.is_contiguous())


class AdamW(torch.optim.AdamW):
    """``torch.optim.AdamW`` whose ``step()`` runs as native multi-tensor launches where the module docstring's conditions hold."""

    def _collect(self):
        """One pass over the parameters that have a gradient -> None where the step is torch's, else (device index or None
        without any gradient, [(group, [(p, grad, exp_avg, exp_avg_sq, step)])], whether every such parameter has its state)."""
        idx, out, complete = None, [], True
        checked = self.__dict__.setdefault("_checked_states", {})
        for group in self.param_groups:
            if (group["amsgrad"] or group["maximize"] or group["capturable"] or group["differentiable"] or group["fused"]
                    or not group.get("decoupled_weight_decay", True)):
                return None
            if any(isinstance(group[k], torch.Tensor) for k in ("lr", "eps", "weight_decay")) or any(
                    isinstance(b, torch.Tensor) for b in group["betas"]):
                return None
            entries = []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if idx is None:
                    if not p.is_cuda:
                        return None
                    idx = p.get_device()
                if not (_dense_f32(p, idx) and _dense_f32(g, idx)):
                    return None
                st = self.state.get(p)
                if not st:
                    complete = False
                    continue
                m, v, step = st["exp_avg"], st["exp_avg_sq"], st["step"]
                seen = checked.get(p)
                if seen is None or seen[0] is not m or seen[1] is not v or seen[2] is not step or seen[3] != idx:
                    if not (_dense_f32(m, idx) and _dense_f32(v, idx) and isinstance(step, torch.Tensor) and step.dtype is torch.float32
                            and not step.is_cuda and step.dim() == 0):
                        return None
                    checked[p] = (m, v, step, idx)        # the optimizer's own tensors: checked once per object, not per step
                entries.append((p, g, m, v, step))
            out.append((group, entries))
        return idx, out, complete

    def _native_device(self):
        """The device of a native step, or None where the step is torch's."""
        plan = self._collect()
        return None if plan is None or plan[0] is None else torch.device("cuda", plan[0])

    def _count_steps(self, key, entries):
        """Increments the entries' ``step`` tensors and returns the new numbers.  The steps of a group live as 0-dim views of one
        flat CPU tensor (still CPU fp32 tensors in ``state`` and ``state_dict()``), so that counting a step is one add and one
        read for the list instead of one of each per parameter; the views are rebuilt whenever the list or a tensor changed."""
        flats = self.__dict__.setdefault("_step_flats", {})
        flat = flats.get(key)
        base = flat.data_ptr() if flat is not None and flat.numel() == len(entries) else None
        if base is None or any(e[4].data_ptr() != base + 4 * i for i, e in enumerate(entries)):
            flat = flats[key] = torch.stack([e[4] for e in entries])
            for i, e in enumerate(entries):
                self.state[e[0]]["step"] = flat[i]
        flat += 1
        return [int(s) for s in flat.tolist()]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan = self._collect()
        if plan is not None and plan[0] is not None and not plan[2]:
            for group in self.param_groups:               # the missing states, created as the parent creates them
                self._init_group(group, [], [], [], [], [], [])
            plan = self._collect()
        if plan is None or plan[0] is None:
            parent = torch.optim.AdamW.step
            if getattr(parent, "hooked", False):          # torch wrapped the parent's step with the step hooks for another
                parent = parent.__wrapped__               # instance; this class's own step already runs them once
            parent(self)
            return loss
        lib = _lib.load()
        dev = torch.device("cuda", plan[0])
        updated = []
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for key, (group, entries) in enumerate(plan[1]):
                if not entries:
                    continue
                steps = self._count_steps(key, entries)
                rows = [(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), s)
                        for (p, g, m, v, _), s in zip(entries, steps) if p.numel() > 0]        # an empty parameter counts its step, no more
                if not rows:
                    continue
                n = len(rows)
                cols = list(zip(*rows))
                ptr_t, i64_t = ctypes.c_void_p * n, ctypes.c_int64 * n
                beta1, beta2 = group["betas"]
                _check(lib.st_adamw_step(ptr_t(*cols[0]), ptr_t(*cols[1]), ptr_t(*cols[2]), ptr_t(*cols[3]), i64_t(*cols[4]), i64_t(*cols[5]),
                                         n, float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]),
                                         stream))
                updated += [e[0] for e in entries if e[0].numel() > 0]
        # the kernels wrote through raw pointers: tell autograd, and with it the native modules' weight caches (_param_key)
        updated = [p for p in updated if not p.is_inference()]
        if updated:
            torch.autograd.graph.increment_version(updated)
        return loss


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_``: scales the gradients in place so that their total norm is at most ``max_norm`` and
    returns the total norm before clipping, a 0-dim fp32 tensor on the gradients' device."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    else:
        parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    full = [g for g in grads if g.numel() > 0]
    native = bool(full) and float(norm_type) == 2.0 and not error_if_nonfinite and full[0].is_cuda
    if native:
        dev = full[0].device
        native = all(_dense_f32(g, dev.index) for g in grads)
    if not native:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite,
                                              foreach=foreach)
    lib = _lib.load()
    n = len(full)
    ptrs, counts = _ptrs(full), _counts(full)
    nbytes = int(lib.st_grad_norm_scratch_bytes(counts, n))
    if nbytes < 0:
        _check(nbytes)
    total_norm = torch.empty((), device=dev, dtype=torch.float32)
    scratch = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(lib.st_grad_norm(ptrs, counts, n, total_norm.data_ptr(), scratch.data_ptr(), nbytes, stream))
        _check(lib.st_grad_clip(ptrs, counts, n, total_norm.data_ptr(), float(max_norm), stream))
    return total_norm
