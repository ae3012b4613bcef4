"""Duration -> alignment -> ``mu_y`` of ``StableTTS.synthesise`` (models/model.py:82-96) on native gfx950 kernels
(SURVEY.md section 8f-3): the step between the TextEncoder and the CFM decoder.

``generate_path(duration, mask)`` is a drop-in for the reference's module-level function (models/model.py:17-27);
``length_regulate(logw, x_mask, mu_x, length_scale)`` performs lines 85-95 -- ``w_ceil``, ``y_lengths``, ``y_mask``,
the alignment and ``mu_y = attn^T mu_x`` -- with the matmul replaced by the gather it is (the alignment has exactly
one 1 per mel frame).  Integer / index results are bit-exact with the reference for exactly summable durations.

The training side of the same step, monotonic alignment search (models/model.py:148-162): ``maximum_path(neg_cent, t_y,
t_x)`` runs monotonic_align's dynamic program and backtrack on the device (bit-exact), and
``monotonic_alignment(mu_x, x_mask, y, y_mask)`` adds the fused ``neg_cent`` in front and ``logw_`` behind it.
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
    logw_ (B, 1, Tx) = log(1e-8 + durations) * x_mask).  mu_y stays the caller's matmul (gradients reach mu_x through it):
    mu_y = torch.matmul(attn.squeeze(1).transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)."""
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
