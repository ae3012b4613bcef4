"""Duration -> alignment -> ``mu_y`` of ``StableTTS.synthesise`` (models/model.py:82-96) on native gfx950 kernels
(SURVEY.md section 8f-3): the step between the TextEncoder and the CFM decoder.

``generate_path(duration, mask)`` is a drop-in for the reference's module-level function (models/model.py:17-27);
``length_regulate(logw, x_mask, mu_x, length_scale)`` performs lines 85-95 -- ``w_ceil``, ``y_lengths``, ``y_mask``,
the alignment and ``mu_y = attn^T mu_x`` -- with the matmul replaced by the gather it is (the alignment has exactly
one 1 per mel frame).  Integer / index results are bit-exact with the reference for exactly summable durations.

The training side of the same step, monotonic alignment search (models/model.py:148-162): ``maximum_path(neg_cent, t_y,
t_x)`` runs monotonic_align's dynamic program and backtrack on the device (bit-exact), and
``monotonic_alignment(mu_x, x_mask, y, y_mask)`` adds the fused ``neg_cent`` in front and ``logw_`` behind it.
``align_and_losses(...)`` is everything behind the search (models/model.py:160-176 without the decoder call): ``mu_y`` as a
gather, ``mu_y_masked``, ``prior_loss``, ``logw_`` and ``dur_loss`` from the per-token frame counts, differentiable in
``mu_x``, ``logw`` and ``fake_content`` (d ``mu_x`` is a segmented sum); no dense alignment exists on that path, and
``dense_alignment(frame_token, Tx)`` builds one only for a caller who wants to look at it.
There is no CPU fallback.
"""
import ctypes

import torch

from . import _lib


def _check(rc):
    if rc != _lib.ST_OK:
        raise _lib.NativeError(rc, _lib.load().st_last_error(None).decode())


def _dev(t, name):
    if t.device.type != "cuda":
        raise RuntimeError(f"stabletts_amd: {name} must be on a HIP device (there is no CPU fallback)")
    return t.device


def generate_path(duration, mask):
    """models/model.py:17-27.  duration (B, Tx) fp32, mask (B, Tx, Ty) -> path (B, Tx, Ty) of mask.dtype."""
    lib = _lib.load()
    dev = _dev(duration, "duration")
    b, t_x, t_y = mask.shape
    d = duration.detach().to(dtype=torch.float32).contiguous()
    m = mask.detach().to(device=dev, dtype=torch.float32).contiguous()
    cum = torch.empty(b, t_x, device=dev, dtype=torch.float32)
    path = torch.empty(b, t_x, t_y, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _check(lib.st_generate_path(d.data_ptr(), m.data_ptr(), b, t_x, t_y, cum.data_ptr(), path.data_ptr(),
                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return path.to(mask.dtype)


@torch.no_grad()
def length_regulate(logw, x_mask, mu_x, length_scale=1.0, return_attn=True):
    """models/model.py:85-95.  logw, x_mask (B, 1, Tx); mu_x (B, M, Tx) ->
    dict(w_ceil (B,1,Tx), y_lengths (B,) long, y_mask (B,1,Ty), attn (B,1,Tx,Ty) or None, mu_y (B,M,Ty))."""
    lib = _lib.load()
    dev = _dev(logw, "logw")
    B, _, Tx = logw.shape
    M = mu_x.shape[1]
    lw = logw.detach().to(dtype=torch.float32).contiguous()
    xm = x_mask.detach().to(device=dev, dtype=torch.float32).contiguous()
    mx = mu_x.detach().to(device=dev, dtype=torch.float32).contiguous()
    w_ceil = torch.empty(B, 1, Tx, device=dev, dtype=torch.float32)
    cum = torch.empty(B, Tx, device=dev, dtype=torch.float32)
    y_lengths = torch.empty(B, device=dev, dtype=torch.long)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        _check(lib.st_durations(lw.data_ptr(), xm.data_ptr(), float(length_scale), B, Tx, w_ceil.data_ptr(), cum.data_ptr(),
                                y_lengths.data_ptr(), stream))
        Ty = int(y_lengths.max())                   # the reference synchronises here too (model.py:88)
        mu_y = torch.empty(B, M, Ty, device=dev, dtype=torch.float32)
        y_mask = torch.empty(B, 1, Ty, device=dev, dtype=torch.float32)
        attn = torch.empty(B, 1, Tx, Ty, device=dev, dtype=torch.float32) if return_attn else None
        _check(lib.st_align(cum.data_ptr(), xm.data_ptr(), y_lengths.data_ptr(), mx.data_ptr(), B, M, Tx, Ty,
                            attn.data_ptr() if attn is not None else None, mu_y.data_ptr(), y_mask.data_ptr(), stream))
    return dict(w_ceil=w_ceil, y_lengths=y_lengths, y_mask=y_mask, attn=attn, mu_y=mu_y)


def maximum_path(neg_cent, t_y, t_x, durations=False):
    """monotonic_align/core.py:14-46 on the device.  neg_cent (B, Ty, Tx) fp32 (converted if not), t_y / t_x (B) lengths
    (any integer or float dtype, truncated to int32) -> path (B, Ty, Tx) fp32 0/1, and with durations=True also the
    frames per token (B, Tx) int32.  neg_cent is not modified; nothing is read back to the host."""
    lib = _lib.load()
    dev = _dev(neg_cent, "neg_cent")
    B, Ty, Tx = neg_cent.shape
    nc = neg_cent.detach().to(dtype=torch.float32).contiguous()
    ty = t_y.detach().to(device=dev, dtype=torch.int32).contiguous()
    tx = t_x.detach().to(device=dev, dtype=torch.int32).contiguous()
    path = torch.empty(B, Ty, Tx, device=dev, dtype=torch.float32)
    dur = torch.empty(B, Tx, device=dev, dtype=torch.int32) if durations else None
    nws = int(lib.st_maximum_path_workspace_bytes(B, Ty, Tx))
    ws = torch.empty(nws, device=dev, dtype=torch.uint8) if nws else None
    with torch.cuda.device(dev):
        _check(lib.st_maximum_path(nc.data_ptr(), ty.data_ptr(), tx.data_ptr(), B, Ty, Tx, path.data_ptr(),
                                   dur.data_ptr() if dur is not None else None, ws.data_ptr() if ws is not None else None,
                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return (path, dur) if durations else path


def mas_neg_cent(mu_x, y):
    """models/model.py:150-155 (s_p_sq_r = 1): mu_x (B, D, Tx), y (B, D, Ty) -> neg_cent (B, Ty, Tx) fp32."""
    lib = _lib.load()
    dev = _dev(mu_x, "mu_x")
    B, D, Tx = mu_x.shape
    Ty = y.shape[2]
    mx = mu_x.detach().to(dtype=torch.float32).contiguous()
    yy = y.detach().to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty(B, Ty, Tx, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _check(lib.st_mas_neg_cent(mx.data_ptr(), yy.data_ptr(), B, D, Tx, Ty, out.data_ptr(),
                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out


@torch.no_grad()
def monotonic_alignment(mu_x, x_mask, y, y_mask):
    """models/model.py:148-162 without the host round trip.  mu_x (B, D, Tx), x_mask (B, 1, Tx), y (B, D, Ty),
    y_mask (B, 1, Ty) -> dict(attn (B, 1, Ty, Tx) fp32 0/1, durations (B, 1, Tx) fp32 = attn.sum(2),
    logw_ (B, 1, Tx) = log(1e-8 + durations) * x_mask).  mu_y is either the caller's matmul (gradients reach mu_x through it),
    mu_y = torch.matmul(attn.squeeze(1).transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2), or, without the dense
    alignment, ``align_and_losses(..., durations=out["durations"])``."""
    _dev(mu_x, "mu_x")
    neg_cent = mas_neg_cent(mu_x, y)
    # the reference's attn_mask = x_mask[:, :, None] * y_mask[..., None] summed over one axis (model.py:157, core.py
    # callers), without materialising the (B, Ty, Tx) mask
    xm, ym = x_mask[:, 0].to(torch.float32), y_mask[:, 0].to(device=mu_x.device, dtype=torch.float32)
    t_y = (xm[:, :1] * ym).sum(1)
    t_x = (xm * ym[:, :1]).sum(1)
    path, dur = maximum_path(neg_cent, t_y, t_x, durations=True)
    durations = dur.to(torch.float32).unsqueeze(1)
    logw_ = torch.log(1e-8 + durations) * x_mask
    return dict(attn=path.unsqueeze(1), durations=durations, logw_=logw_)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _AlignLossFn(torch.autograd.Function):
    """models/model.py:162-163, 166-168, 171-172 and 175-176 on st_align_train_forward / st_duration_loss, and their
    gradients on st_align_train_backward / st_duration_loss_backward.  Inputs (mu_x, logw, fake_content or None, then data:
    x_mask, x_lengths, y, y_mask, durations int32, keep or None); outputs (mu_y, mu_y_masked, prior_loss, dur_loss, logw_,
    frame_token), the last two not differentiable."""

    @staticmethod
    def forward(ctx, mu_x, logw, fake_content, x_mask, x_lengths, y, y_mask, dur, keep):
        lib = _lib.load()
        dev = mu_x.device
        B, M, Tx = mu_x.shape
        Ty = y.shape[2]
        f32 = dict(device=dev, dtype=torch.float32)
        mx = mu_x.detach().to(torch.float32).contiguous()
        lw = logw.detach().to(**f32).contiguous()
        fc = fake_content.detach().to(**f32).reshape(-1).contiguous() if fake_content is not None else None
        xm, ym = x_mask.detach().to(**f32).contiguous(), y_mask.detach().to(**f32).contiguous()
        yy = y.detach().to(**f32).contiguous()
        xl = x_lengths.detach().to(device=dev, dtype=torch.long).contiguous()
        kp = keep.detach().to(**f32).reshape(-1).contiguous() if keep is not None else None
        if (yy.shape != (B, M, Ty) or lw.numel() != B * Tx or xm.numel() != B * Tx or ym.numel() != B * Ty or dur.shape != (B, Tx)
                or xl.numel() != B or (fc is not None and fc.numel() != M) or (kp is not None and kp.numel() != B)):
            raise ValueError("shape mismatch: mu_x (B, M, Tx), y (B, M, Ty), logw / x_mask (B, 1, Tx), y_mask (B, 1, Ty), "
                             "durations (B, Tx), x_lengths (B), fake_content M values, keep B values")
        nscr = int(lib.st_align_train_scratch_floats(B, M, Ty))
        if nscr < 0:
            raise ValueError("shape out of range")
        frame_token = torch.empty(B, Ty, device=dev, dtype=torch.int32)
        mu_y, mu_y_masked = torch.empty(B, M, Ty, **f32), torch.empty(B, M, Ty, **f32)
        scratch = torch.empty(nscr, **f32)
        dscratch = torch.empty(int(lib.st_duration_loss_scratch_floats()), **f32)
        prior, dloss = torch.empty((), **f32), torch.empty((), **f32)
        logw_ = torch.empty(B, 1, Tx, **f32)
        with torch.cuda.device(dev):
            s = _stream(dev)
            _check(lib.st_align_train_forward(dur.data_ptr(), xm.data_ptr(), ym.data_ptr(), mx.data_ptr(), yy.data_ptr(), _ptr(fc),
                                              _ptr(kp), B, M, Tx, Ty, frame_token.data_ptr(), mu_y.data_ptr(), mu_y_masked.data_ptr(),
                                              scratch.data_ptr(), prior.data_ptr(), s))
            _check(lib.st_duration_loss(lw.data_ptr(), dur.data_ptr(), xm.data_ptr(), xl.data_ptr(), B, Tx, logw_.data_ptr(),
                                        dscratch.data_ptr(), dloss.data_ptr(), s))
        ctx.save_for_backward(mx, lw, xm, ym, yy, dur, kp, scratch, dscratch)
        ctx.fake_shape = tuple(fake_content.shape) if fake_content is not None else None
        ctx.mark_non_differentiable(logw_, frame_token)
        ctx.set_materialize_grads(False)
        return mu_y, mu_y_masked, prior, dloss, logw_, frame_token

    @staticmethod
    def backward(ctx, g_mu_y, g_masked, g_prior, g_dur, _g_logw_, _g_tok):
        lib = _lib.load()
        mx, lw, xm, ym, yy, dur, kp, scratch, dscratch = ctx.saved_tensors
        dev = mx.device
        B, M, Tx = mx.shape
        Ty = yy.shape[2]
        f32 = dict(device=dev, dtype=torch.float32)
        prep = lambda g, n: g.detach().to(**f32).reshape(n).contiguous() if g is not None else None      # noqa: E731
        g_mu_y, g_masked = prep(g_mu_y, (B, M, Ty)), prep(g_masked, (B, M, Ty))
        g_prior, g_dur = prep(g_prior, 1), prep(g_dur, 1)
        need_mu, need_logw, need_fc = ctx.needs_input_grad[:3]
        grad_mu_x = grad_logw = grad_fc = None
        with torch.cuda.device(dev):
            s = _stream(dev)
            if (need_mu or need_fc) and (g_mu_y is not None or g_masked is not None or g_prior is not None):
                grad_mu_x = torch.empty_like(mx)
                grad_fc = torch.empty(M, **f32) if need_fc and ctx.fake_shape is not None else None
                _check(lib.st_align_train_backward(dur.data_ptr(), xm.data_ptr(), ym.data_ptr(), mx.data_ptr(), yy.data_ptr(), _ptr(kp),
                                                   scratch.data_ptr(), _ptr(g_masked), _ptr(g_mu_y), _ptr(g_prior), B, M, Tx, Ty,
                                                   grad_mu_x.data_ptr(), _ptr(grad_fc), s))
                if grad_fc is not None:
                    grad_fc = grad_fc.reshape(ctx.fake_shape)
                if not need_mu:
                    grad_mu_x = None
            if need_logw and g_dur is not None:
                grad_logw = torch.empty_like(lw)
                _check(lib.st_duration_loss_backward(lw.data_ptr(), dur.data_ptr(), xm.data_ptr(), dscratch.data_ptr(), g_dur.data_ptr(),
                                                     B, Tx, grad_logw.data_ptr(), s))
        return grad_mu_x, grad_logw, grad_fc, None, None, None, None, None, None


def align_and_losses(mu_x, x_mask, logw, x_lengths, y, y_mask, durations, keep=None, fake_content=None):
    """models/model.py:160-176 around the decoder call, from the frame counts of the alignment search.  mu_x (B, M, Tx),
    x_mask / logw (B, 1, Tx), x_lengths (B), y (B, M, Ty), y_mask (B, 1, Ty); durations (B, Tx) or (B, 1, Tx), int32 as
    maximum_path(..., durations=True) returns them or the fp32 ``durations`` of monotonic_alignment; keep: the cfg_mask of
    :138 (B values, non-zero keeps the content; None keeps all); fake_content (1, M, 1) or None (= 0).
    -> dict(mu_y, mu_y_masked (B, M, Ty), prior_loss, dur_loss (scalars), logw_ (B, 1, Tx), frame_token (B, Ty) int32, -1
    where no token covers the frame).  Gradients reach mu_x (through mu_y, mu_y_masked and prior_loss), logw and fake_content.
    No host synchronisation, no dense alignment."""
    dev = _dev(mu_x, "mu_x")
    B, _, Tx = mu_x.shape
    dur = durations.detach().to(device=dev).reshape(B, Tx).to(torch.int32).contiguous()
    mu_y, mu_y_masked, prior, dloss, logw_, frame_token = _AlignLossFn.apply(mu_x, logw, fake_content, x_mask, x_lengths, y, y_mask,
                                                                             dur, keep)
    return dict(mu_y=mu_y, mu_y_masked=mu_y_masked, prior_loss=prior, dur_loss=dloss, logw_=logw_, frame_token=frame_token)


def dense_alignment(frame_token, Tx):
    """frame_token (B, Ty) as align_and_losses returns it -> the 0/1 alignment (B, Tx, Ty) fp32, the fourth value
    StableTTS.forward returns (models/model.py:166, 178).  Only for callers who want to look at it: nothing computes with it."""
    B, Ty = frame_token.shape
    attn = torch.zeros(B, Tx + 1, Ty, device=frame_token.device, dtype=torch.float32)
    idx = torch.where(frame_token < 0, Tx, frame_token).to(torch.long).unsqueeze(1)      # uncovered frames go to a spare row
    return attn.scatter_(1, idx, 1.0)[:, :Tx]
