"""Drop-in replacement for the reference's ``monotonic_align`` package (monotonic_align/__init__.py:7-16), the one
``models/model.py:5`` imports for StableTTS's training forward.

``maximum_path(neg_cent, mask)`` keeps the reference's signature and result -- the (B, Ty, Tx) 0/1 path in
``neg_cent.dtype`` on ``neg_cent.device`` -- but runs the dynamic program and the backtrack on gfx950
(``st_maximum_path``, include/stabletts_hip.h): no device-to-host copy of ``neg_cent``, no host synchronisation, no numba.
Any float dtype is accepted and converted to fp32 like the reference's ``astype(float32)``; the lengths come from the
reference's own expressions, evaluated on the device.  Bit-exact with the reference for every item with t_x, t_y >= 1;
an item with t_x == 0 or t_y == 0 gets an all-zero path.  There is no CPU fallback: CPU tensors raise.
"""
import torch

from .alignment import maximum_path as _maximum_path

__all__ = ["maximum_path"]


@torch.no_grad()
def maximum_path(neg_cent, mask):
    """neg_cent (B, Ty, Tx), mask (B, Ty, Tx) -> path (B, Ty, Tx) of neg_cent.dtype (monotonic_align/__init__.py:7)."""
    if neg_cent.device.type != "cuda":
        raise RuntimeError("stabletts_amd: neg_cent must be on a HIP device (there is no CPU fallback)")
    t_y = mask.sum(1)[:, 0]
    t_x = mask.sum(2)[:, 0]
    path = _maximum_path(neg_cent, t_y, t_x)
    return path.to(dtype=neg_cent.dtype)
