"""float64 numpy restatement of the alignment training kernels (stabletts_amd/csrc/align_train_kernels.hip): the index map
from the frame counts, the gather, both losses of models/model.py:162-176 and their gradients as segmented sums, plus the
quantities the error bounds of the GPU tests are made of.  Loops are plain Python: the shapes of the tests are small.
Not a test module."""
import math
import os

import numpy as np

LOG_2PI = math.log(2 * math.pi)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_loss_grads.npz")
CASES = ("ragged", "wide", "edges_dropped", "edges_kept")


def case_of(gold, name):
    """gold: dict(np.load(GOLDEN)).  The case's arrays plus its masks; float32 inputs are also given in float64 under <key>64."""
    g = {k[len(name) + 1:]: v for k, v in gold.items() if k.startswith(name + "/")}
    B, M, Tx = g["mu_x"].shape
    Ty = g["y"].shape[2]
    g["x_mask"] = (np.arange(Tx)[None] < g["x_lengths"][:, None]).astype(np.float32)[:, None]
    g["y_mask"] = (np.arange(Ty)[None] < g["y_lengths"][:, None]).astype(np.float32)[:, None]
    for k in ("mu_x", "logw", "y", "W", "fake_content", "x_mask", "y_mask"):
        g[k + "64"] = g[k].astype(np.float64)
    return g


def segment_ends(durations, x_mask, Ty):
    """durations (B, Tx) integers, x_mask (B, 1, Tx) or (B, Tx) -> ends (B, Tx) int64: token i owns the frames
    [ends[i-1], ends[i]).  This DEFINES the clipping: a token counts only where x_mask != 0, a negative count is 0, a count is
    at most Ty, and the running sum is clipped to Ty."""
    d = np.asarray(durations).astype(np.int64)
    xm = np.asarray(x_mask).reshape(d.shape) != 0
    d = np.where(xm, np.clip(d, 0, Ty), 0)
    return np.minimum(np.cumsum(d, axis=1), Ty)


def frame_token(durations, x_mask, Ty):
    """-> (B, Ty) int32: the token of each frame, -1 where no token covers it."""
    ends = segment_ends(durations, x_mask, Ty)
    B, Tx = ends.shape
    tok = np.full((B, Ty), -1, np.int32)
    for b in range(B):
        s = 0
        for i in range(Tx):
            tok[b, s:ends[b, i]] = i
            s = ends[b, i]
    return tok


def forward(mu_x, x_mask, logw, x_lengths, y, y_mask, durations, keep=None, fake_content=None):
    """All arrays float64 (durations integer).  -> dict(frame_token, mu_y, mu_y_masked, prior_loss, dur_loss, logw_)."""
    B, M, Tx = mu_x.shape
    Ty = y.shape[2]
    tok = frame_token(durations, x_mask, Ty)
    mu_y = np.zeros((B, M, Ty))
    for b in range(B):
        hit = tok[b] >= 0
        mu_y[b][:, hit] = mu_x[b][:, tok[b][hit]]
    k = np.ones(B) if keep is None else (np.asarray(keep).reshape(B) != 0).astype(np.float64)
    fc = np.zeros(M) if fake_content is None else np.asarray(fake_content, np.float64).reshape(M)
    mu_y_masked = mu_y * k[:, None, None] + (1 - k)[:, None, None] * fc[None, :, None]
    ym = np.asarray(y_mask, np.float64).reshape(B, 1, Ty)
    prior = np.sum(0.5 * ((y - mu_y) ** 2 + LOG_2PI) * ym) / (np.sum(ym) * M)
    d = np.maximum(np.asarray(durations).reshape(B, 1, Tx).astype(np.float64), 0)
    logw_ = np.log(1e-8 + d) * np.asarray(x_mask, np.float64).reshape(B, 1, Tx)
    dur = np.sum((np.asarray(logw, np.float64).reshape(B, 1, Tx) - logw_) ** 2) / float(np.sum(x_lengths))
    return dict(frame_token=tok, mu_y=mu_y, mu_y_masked=mu_y_masked, prior_loss=prior, dur_loss=dur, logw_=logw_)


def backward(mu_x, x_mask, logw, x_lengths, y, y_mask, durations, keep=None, g_masked=None, g_mu_y=None, g_prior=None, g_dur=None):
    """Gradients of sum(g_masked * mu_y_masked) + sum(g_mu_y * mu_y) + g_prior * prior_loss + g_dur * dur_loss.
    -> dict(grad_mu_x (B, M, Tx), grad_logw (B, 1, Tx), grad_fake_content (M),
            n (B, Tx): frames per token after clipping,  S (B, M, Tx): the sum of |term| over the terms of grad_mu_x's sum,
            n_fake: (terms a thread sums, terms of the tree), S_fake (M): the sum of |term| of grad_fake_content)."""
    B, M, Tx = mu_x.shape
    Ty = y.shape[2]
    ends = segment_ends(durations, x_mask, Ty)
    k = np.ones(B) if keep is None else (np.asarray(keep).reshape(B) != 0).astype(np.float64)
    ym = np.asarray(y_mask, np.float64).reshape(B, Ty)
    denom = np.sum(ym) * M
    zero = np.zeros((B, M, Ty))
    gm = zero if g_masked is None else np.asarray(g_masked, np.float64)
    gy = zero if g_mu_y is None else np.asarray(g_mu_y, np.float64)
    gp = 0.0 if g_prior is None else float(g_prior)
    grad = np.zeros((B, M, Tx))
    S = np.zeros((B, M, Tx))
    n = np.zeros((B, Tx), np.int64)
    for b in range(B):
        s = 0
        for i in range(Tx):
            e = int(ends[b, i])
            n[b, i] = e - s
            for t in range(s, e):                                   # ascending t, one fixed order
                term = k[b] * gm[b, :, t] + gy[b, :, t] + gp * ym[b, t] * (mu_x[b, :, i] - y[b, :, t]) / denom
                grad[b, :, i] += term
                S[b, :, i] += np.abs(term)
            s = e
    dropped = k == 0
    grad_fc = gm[dropped].sum(axis=(0, 2)) if dropped.any() else np.zeros(M)
    S_fake = np.abs(gm[dropped]).sum(axis=(0, 2)) if dropped.any() else np.zeros(M)
    n_fake = (int(dropped.sum()) * ((Ty + 255) // 256), 256)
    d = np.maximum(np.asarray(durations).reshape(B, 1, Tx).astype(np.float64), 0)
    logw_ = np.log(1e-8 + d) * np.asarray(x_mask, np.float64).reshape(B, 1, Tx)
    gd = 0.0 if g_dur is None else float(g_dur)
    grad_logw = gd * 2 * (np.asarray(logw, np.float64).reshape(B, 1, Tx) - logw_) / float(np.sum(x_lengths))
    return dict(grad_mu_x=grad, grad_logw=grad_logw, grad_fake_content=grad_fc, n=n, S=S, n_fake=n_fake, S_fake=S_fake)
