"""Row-vectorised numpy restatement of monotonic alignment search (the reference's monotonic_align/core.py:14-46), so that
tests can check shapes far beyond what the pure-Python reference can sweep.  Same fp32 arithmetic: within a row every
band cell depends only on the row above, so a row is one vectorised step; the backtrack is the reference's loop.

    path = maximum_path(neg_cent, t_y, t_x)      # neg_cent (B, Ty, Tx), lengths (B,) -> (B, Ty, Tx) int32 0/1

An item with t_x == 0 or t_y == 0 gets an all-zero path (the reference writes through a negative index there).
"""
import numpy as np

MAX_NEG = np.float32(-1e9)


def dp_values(value, t_y, t_x):
    """The forward pass of maximum_path_jit on one item: value (Ty, Tx) fp32, accumulated in place inside the band."""
    for y in range(t_y):
        lo, hi = max(0, t_x + y - t_y), min(t_x, y + 1)
        if hi <= lo:
            continue
        xs = np.arange(lo, hi)
        if y == 0:
            v_cur = np.full(xs.shape, MAX_NEG, np.float32)             # x == y == 0
            v_prev = np.zeros(xs.shape, np.float32)
        else:
            above = value[y - 1]
            v_cur = np.where(xs == y, MAX_NEG, above[xs]).astype(np.float32)
            v_prev = np.where(xs == 0, MAX_NEG, above[np.maximum(xs - 1, 0)]).astype(np.float32)
        m = np.where(v_cur > v_prev, v_cur, v_prev)                      # Python's max(v_prev, v_cur)
        value[y, lo:hi] = value[y, lo:hi] + m                            # fp32 add
    return value


def backtrack(value, t_y, t_x):
    """Path columns per row (t_y,) of an accumulated value table (maximum_path_jit's second loop)."""
    cols = np.zeros(t_y, np.int64)
    index = t_x - 1
    for y in range(t_y - 1, -1, -1):
        cols[y] = index
        if index != 0 and (index == y or value[y - 1, index] < value[y - 1, index - 1]):
            index -= 1
    return cols


def maximum_path(neg_cent, t_y, t_x):
    neg_cent = np.asarray(neg_cent, dtype=np.float32)
    B, Ty, Tx = neg_cent.shape
    path = np.zeros((B, Ty, Tx), np.int32)
    for b in range(B):
        ty, tx = int(t_y[b]), int(t_x[b])
        if ty <= 0 or tx <= 0:
            continue
        value = dp_values(neg_cent[b].copy(), ty, tx)
        path[b, np.arange(ty), backtrack(value, ty, tx)] = 1
    return path


def lengths_from_mask(mask):
    """The reference's t_y, t_x (monotonic_align/__init__.py:13-14): mask (B, Ty, Tx) -> int32 (B,), (B,)."""
    mask = np.asarray(mask)
    return mask.sum(1)[:, 0].astype(np.int32), mask.sum(2)[:, 0].astype(np.int32)
