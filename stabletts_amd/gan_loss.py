"""The three scalar GAN losses of a Vocos training step (vocoders/vocos/models/loss.py:37-66) on native gfx950 kernels:
``feature_loss(fmap_r, fmap_g)``, ``discriminator_loss(disc_real_outputs, disc_generated_outputs)`` and
``generator_loss(disc_outputs)``, with the reference's signatures and return structures.  ``install(gan_losses=True)`` rebinds the
three names inside the user's ``vocoders.vocos.models.loss``.

Each call is ONE autograd node over the flattened list: a multi-tensor forward (``st_feature_loss_forward`` /
``st_lsgan_loss_forward``: per-tensor means and their sum, fp64 accumulation in one fixed order, no atomics, bitwise repeatable)
and one elementwise multi-tensor backward that reads the upstream gradient on the device.  ``discriminator_loss`` reads its two
lists of floats with one device-to-host copy instead of one ``.item()`` per value.

The native discriminators run once on ``cat([y, y_hat])`` and return each map's halves as ``f[:n]`` / ``f[n:]``.  Where a pair
(or a real / generated logit pair) tiles one such base, the node takes the BASE as its differentiable input and returns one
gradient tensor for it, written by the one backward kernel -- autograd's zero-fill and add per slice do not happen.  Any other
pair takes the general path; both give the same bits, forward and backward.

The native path runs when every tensor is a CUDA fp32 tensor (non-contiguous ones are made contiguous) and each pair agrees in
shape.  For CPU tensors, other dtypes, an empty tensor or an empty list the functions evaluate the plain expressions in torch, so
the drop-in works everywhere.
"""
import ctypes

import torch

from . import _lib

__all__ = ["feature_loss", "discriminator_loss", "generator_loss"]


def _check(rc):
    if rc != _lib.ST_OK:
        raise _lib.NativeError(rc, _lib.load().st_last_error(None).decode())


def chunk():
    """Elements of one tensor a block of the forward sums (kGanLossChunk)."""
    return int(_lib.load().st_gan_loss_chunk())


def max_pairs():
    """List entries one launch covers (kGanLossMaxPairs)."""
    return int(_lib.load().st_gan_loss_max_pairs())


# ---- the plain expressions (CPU tensors, other dtypes, empty lists)
def _feature_loss_torch(fmap_r, fmap_g):
    loss = 0
    for dr, dg in zip(fmap_r, fmap_g):
        for rl, gl in zip(dr, dg):
            loss = loss + (rl - gl).abs().mean()
    return loss * 2


def _discriminator_loss_torch(disc_real_outputs, disc_generated_outputs):
    loss, r_losses, g_losses = 0, [], []
    for dr, dg in zip(disc_real_outputs, disc_generated_outputs):
        r_loss, g_loss = ((1 - dr) ** 2).mean(), (dg ** 2).mean()
        loss = loss + (r_loss + g_loss)
        r_losses.append(r_loss.item())
        g_losses.append(g_loss.item())
    return loss, r_losses, g_losses


def _generator_loss_torch(disc_outputs):
    loss, gen_losses = 0, []
    for dg in disc_outputs:
        l = ((1 - dg) ** 2).mean()
        gen_losses.append(l)
        loss = loss + l
    return loss, gen_losses


def _native_ok(tensors):
    if not tensors:
        return False
    dev = tensors[0].device
    return all(isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.device == dev and t.dtype == torch.float32
               and t.numel() > 0 for t in tensors)


def _halves_base(a, b):
    """The tensor a and b are the two halves of, or None: both are contiguous views of the same contiguous ``_base``, a starts at
    the base's storage offset, b starts a.numel() after it, and the two counts sum to the base's.  Only where gradients flow to
    both halves through their view nodes (else the general path gives each side its own gradient, or none)."""
    base = a._base
    if base is None or b._base is not base or a.grad_fn is None or b.grad_fn is None or not base.requires_grad:
        return None
    if not (a.requires_grad and b.requires_grad and a.is_contiguous() and b.is_contiguous() and base.is_contiguous()):
        return None
    if base.dtype != a.dtype or a.storage_offset() != base.storage_offset() or b.storage_offset() != a.storage_offset() + a.numel():
        return None
    if a.numel() + b.numel() != base.numel():
        return None
    return base


def _plan(pairs):
    """pairs: [(a, b)] -> (kinds, inputs): kinds[i] is (True, a.numel()) where the node takes the pair's base as ONE input, else
    (False, 0) and it takes a and b."""
    kinds, inputs = [], []
    for a, b in pairs:
        base = _halves_base(a, b) if torch.is_grad_enabled() else None
        if base is not None:
            kinds.append((True, a.numel()))
            inputs.append(base)
        else:
            kinds.append((False, 0))
            inputs += [a, b]
    return kinds, inputs


def _ptr_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _entries(kinds, tensors):
    """-> per list entry (a_ptr, b_ptr, numel, (input index of a, float offset), (input index of b, float offset)) from the
    node's inputs (contiguous fp32)."""
    out, k = [], 0
    for is_base, n_a in kinds:
        if is_base:
            t = tensors[k]
            out.append((t.data_ptr(), t.data_ptr() + 4 * n_a, (n_a, t.numel() - n_a), (k, 0), (k, n_a)))
            k += 1
        else:
            a, b = tensors[k], tensors[k + 1]
            out.append((a.data_ptr(), b.data_ptr(), (a.numel(), b.numel()), (k, 0), (k + 1, 0)))
            k += 2
    return out


def _grad_buffers(tensors, needs):
    """One allocation for the gradients of every input that needs one, each slice on a 256-byte boundary -> [tensor or None]."""
    offs, total = [], 0
    for t, need in zip(tensors, needs):
        offs.append(total if need else None)
        if need:
            total += (t.numel() + 63) // 64 * 64
    if not total:
        return [None] * len(tensors)
    flat = torch.empty(total, device=tensors[0].device, dtype=torch.float32)
    return [None if o is None else flat[o:o + t.numel()].view(t.shape) for t, o in zip(tensors, offs)]


def _forward(kind, mode, ptr_lists, numels, dev):
    """Runs one forward over a list -> out (1 + n floats: the loss, then the means)."""
    lib = _lib.load()
    n = len(numels)
    counts = (ctypes.c_int64 * n)(*numels)
    nbytes = int(lib.st_gan_loss_scratch_bytes(counts, n))
    if nbytes < 0:
        _check(nbytes)
    out = torch.empty(1 + n, device=dev, dtype=torch.float32)
    scratch = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if kind == "feature":
            _check(lib.st_feature_loss_forward(_ptr_array(ptr_lists[0]), _ptr_array(ptr_lists[1]), counts, n, out.data_ptr(),
                                               scratch.data_ptr(), nbytes, stream))
        else:
            _check(lib.st_lsgan_loss_forward(_ptr_array(ptr_lists[0]), counts, n, mode, out.data_ptr(), scratch.data_ptr(), nbytes, stream))
    return out


class _FeatureLossFn(torch.autograd.Function):
    """Inputs (kinds, *tensors): per pair either its base or (r, g) -> (loss 0-dim, means (n), not differentiable)."""

    @staticmethod
    def forward(ctx, kinds, *tensors):
        ts = [t.detach().contiguous() for t in tensors]
        ent = _entries(kinds, ts)
        for a, b, (na, nb), _, _ in ent:
            if na != nb:
                raise ValueError("feature_loss: the two maps of a pair differ in element count")
        out = _forward("feature", 0, ([e[0] for e in ent], [e[1] for e in ent]), [e[2][0] for e in ent], ts[0].device)
        ctx.kinds = kinds
        ctx.save_for_backward(*ts)
        loss, means = out[0], out[1:]
        ctx.mark_non_differentiable(means)
        ctx.set_materialize_grads(False)
        return loss, means

    @staticmethod
    def backward(ctx, g_loss, _g_means):
        ts = ctx.saved_tensors
        needs = ctx.needs_input_grad[1:]
        if g_loss is None or not any(needs):
            return (None,) * (1 + len(ts))
        lib = _lib.load()
        dev = ts[0].device
        ent = _entries(ctx.kinds, ts)
        grads = _grad_buffers(ts, needs)
        gptr = lambda where: None if grads[where[0]] is None else grads[where[0]].data_ptr() + 4 * where[1]      # noqa: E731
        n = len(ent)
        g = g_loss.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        with torch.cuda.device(dev):
            _check(lib.st_feature_loss_backward(_ptr_array([e[0] for e in ent]), _ptr_array([e[1] for e in ent]),
                                                (ctypes.c_int64 * n)(*[e[2][0] for e in ent]), n, g.data_ptr(),
                                                _ptr_array([gptr(e[3]) for e in ent]), _ptr_array([gptr(e[4]) for e in ent]),
                                                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return (None,) + tuple(grads)


class _LsganLossFn(torch.autograd.Function):
    """Inputs (mode, kinds, *tensors).  kinds is None: one tensor per list entry (generator_loss, or either op alone);
    otherwise per (real, generated) pair its base or the two tensors, flattened to the list r_0, g_0, r_1, g_1, ...
    -> (loss 0-dim, means (n), not differentiable)."""

    @staticmethod
    def _list(kinds, ts):
        """-> [(ptr, numel, (input index, float offset))] in list order."""
        if kinds is None:
            return [(t.data_ptr(), t.numel(), (k, 0)) for k, t in enumerate(ts)]
        out = []
        for a, b, (na, nb), wa, wb in _entries(kinds, ts):
            out += [(a, na, wa), (b, nb, wb)]
        return out

    @staticmethod
    def forward(ctx, mode, kinds, *tensors):
        ts = [t.detach().contiguous() for t in tensors]
        lst = _LsganLossFn._list(kinds, ts)
        out = _forward("lsgan", mode, ([e[0] for e in lst],), [e[1] for e in lst], ts[0].device)
        ctx.mode, ctx.kinds = mode, kinds
        ctx.save_for_backward(*ts)
        loss, means = out[0], out[1:]
        ctx.mark_non_differentiable(means)
        ctx.set_materialize_grads(False)
        return loss, means

    @staticmethod
    def backward(ctx, g_loss, _g_means):
        ts = ctx.saved_tensors
        needs = ctx.needs_input_grad[2:]
        if g_loss is None or not any(needs):
            return (None,) * (2 + len(ts))
        lib = _lib.load()
        dev = ts[0].device
        lst = _LsganLossFn._list(ctx.kinds, ts)
        grads = _grad_buffers(ts, needs)
        gptr = lambda where: None if grads[where[0]] is None else grads[where[0]].data_ptr() + 4 * where[1]      # noqa: E731
        n = len(lst)
        g = g_loss.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        with torch.cuda.device(dev):
            _check(lib.st_lsgan_loss_backward(_ptr_array([e[0] for e in lst]), (ctypes.c_int64 * n)(*[e[1] for e in lst]), n, ctx.mode,
                                              g.data_ptr(), _ptr_array([gptr(e[2]) for e in lst]),
                                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return (None, None) + tuple(grads)


def feature_loss(fmap_r, fmap_g):
    """loss.py:37-43: 2 * sum over every (real, generated) feature-map pair of mean|rl - gl| -> a 0-dim tensor, differentiable in
    every map that requires grad (the real maps are not detached, as in the reference)."""
    pairs = [(rl, gl) for dr, dg in zip(fmap_r, fmap_g) for rl, gl in zip(dr, dg)]
    if not _native_ok([t for p in pairs for t in p]) or any(rl.shape != gl.shape for rl, gl in pairs):
        return _feature_loss_torch(fmap_r, fmap_g)
    kinds, inputs = _plan(pairs)
    return _FeatureLossFn.apply(kinds, *inputs)[0]


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    """loss.py:45-56: sum_i mean((1 - dr_i)^2) + mean(dg_i^2) -> (loss, r_losses, g_losses), the two lists Python floats as in
    the reference, read with ONE device-to-host copy of the 2n means (one synchronisation, not 2n)."""
    pairs = list(zip(disc_real_outputs, disc_generated_outputs))
    if not _native_ok([t for p in pairs for t in p]):
        return _discriminator_loss_torch(disc_real_outputs, disc_generated_outputs)
    kinds, inputs = _plan(pairs)
    loss, means = _LsganLossFn.apply(_lib.ST_LSGAN_REAL_FAKE, kinds, *inputs)
    vals = means.tolist()
    return loss, vals[0::2], vals[1::2]


def generator_loss(disc_outputs):
    """loss.py:58-66: sum_i mean((1 - dg_i)^2) -> (loss, gen_losses).  gen_losses is a list of 0-dim tensors that are DETACHED
    views of the node's output buffer: vocoders/vocos/train.py only logs them, and gradients flow through ``loss`` alone."""
    outs = list(disc_outputs)
    if not _native_ok(outs):
        return _generator_loss_torch(disc_outputs)
    loss, means = _LsganLossFn.apply(_lib.ST_LSGAN_REAL, None, *outs)
    means = means.detach()
    return loss, [means[i] for i in range(len(outs))]
