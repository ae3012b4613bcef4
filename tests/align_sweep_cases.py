"""Cases of the alignment sweep (tests/test_align_sweep_cpu.py, tests/test_gpu_mas_sweep.py, tests/test_gpu_align_sweep.py): the
monotonic alignment search on every register plan and both decision-bit stores of mas_path_kernel, the aligned losses at scan
chunks above one token per thread, the duration loss past its grid caps, length regulation past 256 tokens.  Data and small
helpers on the CPU, no GPU work.  Truth is always one of the restatements (tests/mas_restatement.py, tests/align_loss_restatement.py,
tests/align_restatement.py); the references of a case are computed once per process (the search's are handed out read-only).
Not a test module."""
import functools

import numpy as np
import torch

from tests import align_loss_restatement as ar
from tests import mas_restatement as mr

# ---- the launcher's rule (stabletts_amd/csrc/mas_kernels.hip, launch_mas_path), restated
PLANS = (1, 2, 4, 8, 16, 32, 64)                       # K: 64-column groups of state a lane holds
RING = {1: 16, 2: 16, 4: 16, 8: 8, 16: 4, 32: 2, 64: 2}      # P: rows of the prefetch ring
LDS_BUDGET = 65536


def groups_of(Tx):
    return (Tx + 63) // 64


def plan_of(Tx):
    return next(k for k in PLANS if groups_of(Tx) <= k)


def bits_bytes(Ty, Tx):
    return Ty * groups_of(Tx) * 8


def store_of(Ty, Tx):
    return "lds" if bits_bytes(Ty, Tx) <= LDS_BUDGET else "global"


def word_crossings(path, t_y):
    """path (Ty, Tx) 0/1 of one item -> the number of steps that leave column 64 k for column 64 k - 1 (in the backtrack's
    direction), i.e. where the walk changes its decision word."""
    cols = np.asarray(path)[:int(t_y)].argmax(1)
    return int(np.sum((cols[1:] == cols[:-1] + 1) & (cols[1:] % 64 == 0)))


# ---- monotonic alignment search: (Ty, Tx) at B = 3, one row or more per (plan, store)
MAS_TABLE = (
    (65, 64), (64, 63), (8193, 64),
    (130, 65), (4096, 128), (4097, 128),
    (130, 129), (300, 256), (2049, 256),
    (300, 257), (1025, 512),
    (129, 513), (600, 1024),
    (2, 1025), (256, 2048), (257, 2048),
    (128, 4096), (129, 4096), (700, 2049),
)
ON_THE_BUDGET = ((4096, 128), (256, 2048), (128, 4096))       # Ty x groups x 8 B == 65536 exactly
ROW_EDGE_WIDTHS = (130, 600, 2049)                             # rings of 16, 4 and 2 rows
ROW_EDGE_TY = (1, 2, 3, 15, 16, 17, 63, 64, 65)
# one LDS row and one global row of every plan (the poison test), and the rows whose items also run alone
POISON_ROWS = ((65, 64), (8193, 64), (130, 65), (4097, 128), (130, 129), (2049, 256), (300, 257), (1025, 512), (129, 513),
               (600, 1024), (2, 1025), (257, 2048), (128, 4096), (129, 4096))
ALONE_ROWS = ((2049, 256), (600, 1024), (129, 4096))


def mas_id(row):
    Ty, Tx = row
    return f"K{plan_of(Tx)}-{store_of(Ty, Tx)}-{Ty}x{Tx}"


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _randn_rows(B, Ty, Tx, seed):
    """(B, Ty, Tx) fp32 = randn * 4, drawn row by row: two heights at one width and seed share their first rows."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(Ty, B, Tx, generator=gen) * 4).transpose(0, 1).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def mas_case(Ty, Tx):
    """-> neg_cent (3, Ty, Tx) fp32, t_y (3,), t_x (3,) int32.  Item 2 uses only group 0 of a wide plan."""
    t_y = np.array([Ty, max(Ty - 1, 1), Ty // 2 + 1], np.int32)
    t_x = np.array([Tx, max(Tx - 1, 1), min(37, Tx)], np.int32)
    return _frozen(_randn_rows(3, Ty, Tx, 1000 + Tx), t_y, t_x)


@functools.lru_cache(maxsize=None)
def row_edge_case(Tx):
    """B = 9 at tensor height 65: row counts around one ring (P = 16 at Tx = 130) and around one backtrack window (64 rows)."""
    t_y = np.array(ROW_EDGE_TY, np.int32)
    t_x = np.array([min(ty, Tx) - (i & 1) for i, ty in enumerate(ROW_EDGE_TY)], np.int32)
    assert t_x.min() >= 1
    return _frozen(_randn_rows(len(ROW_EDGE_TY), 65, Tx, 2000 + Tx), t_y, t_x)


@functools.lru_cache(maxsize=None)
def ties_case():
    """neg_cent in {-1, 0, 1}: equal neighbours past the first 64-column group; the strict `old < nb` decides them."""
    gen = torch.Generator().manual_seed(3001)
    nc = torch.randint(-1, 2, (2, 200, 130), generator=gen).float().numpy()
    return _frozen(nc, np.array([200, 199], np.int32), np.array([130, 129], np.int32))


@functools.lru_cache(maxsize=None)
def diagonal_case():
    """t_x == t_y = 130: every step of the backtrack is the forced `index == y` move, across two word boundaries."""
    return _frozen(_randn_rows(1, 130, 130, 3002), np.array([130], np.int32), np.array([130], np.int32))


def mas_extra_cases():
    """name -> case function with no arguments, for everything that is not a table row."""
    out = {f"rows-{Tx}": functools.partial(row_edge_case, Tx) for Tx in ROW_EDGE_WIDTHS}
    out["ties"] = ties_case
    out["diagonal"] = diagonal_case
    return out


@functools.lru_cache(maxsize=None)
def _mas_reference(key):
    nc, t_y, t_x = mas_case(*key) if isinstance(key, tuple) else mas_extra_cases()[key]()
    return _frozen(mr.maximum_path(nc, t_y, t_x))[0]


def mas_reference(key):
    """The restatement's path (B, Ty, Tx) int32 of a table row (Ty, Tx) or of an extra case's name, computed once."""
    return _mas_reference(key)


def poisoned(nc, t_y, t_x):
    """A copy of neg_cent with every cell outside [0, t_y) x [0, t_x) of its item set to NaN."""
    out = np.array(nc, copy=True)
    B, Ty, Tx = out.shape
    inside = (np.arange(Ty)[None, :, None] < np.asarray(t_y)[:, None, None]) & (np.arange(Tx)[None, None, :] < np.asarray(t_x)[:, None, None])
    out[~inside] = np.nan
    return out


# ---- the aligned losses: an item is (t_x, t_y, frames of one long token or 0).  An item with t_x > t_y leaves its leading
# tokens without frames (the search starts at token t_x - 1 and drops at most one token a row)
SCAN_CASES = {
    # (B, M, Tx, Ty): items
    (2, 17, 64, 255): ((64, 50, 0), (33, 255, 0)),
    (2, 16, 65, 256): ((65, 40, 0), (30, 256, 0)),
    (2, 80, 256, 257): ((256, 100, 0), (1, 257, 257)),
    (2, 19, 257, 513): ((257, 200, 0), (120, 513, 300)),
    (3, 100, 350, 1000): ((350, 1000, 280), (349, 300, 0), (77, 641, 0)),
    (1, 16, 4096, 4200): ((4096, 4000, 300),),
}
MALFORMED_SHAPE = (2, 19, 257, 513)
CHAIN_SHAPE = (3, 80, 300, 700)
CHAIN_ITEMS = ((300, 655, 0), (211, 700, 0), (1, 9, 9))
DUR_GRID_SHAPES = ((17, 4096), (65, 4096))             # B x Tx > 65536: the forward's stride loop; > 262144: the backward's


def scan_id(shape):
    return "x".join(map(str, shape))


def scan_chunk(Tx):
    """Tokens per thread of the kernels' segment_ends."""
    return (Tx + 255) // 256


def _true_counts(rng, tx, ty, long):
    """Frames per token an utterance is synthesised with: they sum to ty; with tx > ty the leading tokens get none."""
    k = min(tx, ty - max(long - 1, 0))                 # tokens with frames, at the tail
    d = np.ones(k, np.int64)
    if long:
        d[k // 2] = long
    d += rng.multinomial(ty - int(d.sum()), np.full(k, 1.0 / k))
    return np.concatenate([np.zeros(tx - k, np.int64), d])


def _fill64(g):
    for k in ("mu_x", "logw", "y", "W", "fake_content", "x_mask", "y_mask"):
        g[k + "64"] = g[k].astype(np.float64)
    return g


def _case_dict(rng, B, M, Tx, Ty, x_lengths, y_lengths, mu_x, y, logw, durations):
    g = dict(mu_x=mu_x, y=y, logw=logw, durations=durations.astype(np.int32),
             x_lengths=np.asarray(x_lengths, np.int64), y_lengths=np.asarray(y_lengths, np.int64),
             W=(rng.integers(-8, 9, size=(B, M, Ty)) / 4).astype(np.float32),
             fake_content=(rng.standard_normal((1, M, 1)) + np.float32(3)).astype(np.float32),
             keep=np.array([b != 1 for b in range(B)]))          # mixed where B > 1
    g["x_mask"] = (np.arange(Tx)[None] < g["x_lengths"][:, None]).astype(np.float32)[:, None]
    g["y_mask"] = (np.arange(Ty)[None] < g["y_lengths"][:, None]).astype(np.float32)[:, None]
    return _fill64(g)


@functools.lru_cache(maxsize=None)
def aligned_case(shape, items, seed):
    """A case in the layout of align_loss_restatement.case_of: y = expand(mu_x) + 0.3 noise, durations = the frames per token of
    the restatement's alignment search on that pair (the way tools/make_golden_align_losses.py makes a clear alignment)."""
    B, M, Tx, Ty = shape
    assert len(items) == B and max(i[0] for i in items) == Tx and max(i[1] for i in items) <= Ty
    rng = np.random.default_rng(seed)
    mu_x = rng.standard_normal((B, M, Tx)).astype(np.float32)
    y = (rng.standard_normal((B, M, Ty)) * 0.3).astype(np.float32)            # noise alone behind an item's last frame
    logw = np.zeros((B, 1, Tx), np.float32)
    nc = np.zeros((B, Ty, Tx), np.float32)
    for b, (tx, ty, long) in enumerate(items):
        d = _true_counts(rng, tx, ty, long)
        y[b, :, :ty] += mu_x[b][:, np.repeat(np.arange(tx), d)]
        logw[b, 0, :tx] = np.log(np.maximum(d, 0.5)).astype(np.float32) + 0.2 * rng.standard_normal(tx).astype(np.float32)
        yy, mm = y[b, :, :ty], mu_x[b, :, :tx]
        nc[b, :ty, :tx] = -0.5 * (yy ** 2).sum(0)[:, None] + yy.T @ mm - 0.5 * (mm ** 2).sum(0)[None, :]
    t_x, t_y = np.array([i[0] for i in items]), np.array([i[1] for i in items])
    durations = mr.maximum_path(nc, t_y, t_x).sum(1)
    return _case_dict(rng, B, M, Tx, Ty, t_x, t_y, mu_x, y, logw, durations)


def scan_case(shape):
    return aligned_case(shape, SCAN_CASES[shape], 4000 + shape[2])


@functools.lru_cache(maxsize=None)
def duration_grid_case(B, Tx):
    """M = 1, Ty = 8, seeded random counts that sum to at most Ty; logw is non-zero everywhere, behind the mask too, so that
    every element of grad_logw has a non-zero truth."""
    M, Ty = 1, 8
    rng = np.random.default_rng(5000 + B)
    x_lengths = rng.integers(1, Tx + 1, size=B)
    x_lengths[0], x_lengths[-1] = Tx, 1
    durations = np.zeros((B, Tx), np.int64)
    for b in range(B):
        where = rng.choice(x_lengths[b], size=min(3, x_lengths[b]), replace=False)
        durations[b, where] = rng.multinomial(Ty - (b % 3), np.full(len(where), 1.0 / len(where)))
    y_lengths = durations.sum(1)
    y_lengths[0] = Ty
    logw = (rng.standard_normal((B, 1, Tx)) + np.float32(0.25)).astype(np.float32)
    logw[logw == 0] = 1.0
    return _case_dict(rng, B, M, Tx, Ty, x_lengths, y_lengths, rng.standard_normal((B, M, Tx)).astype(np.float32),
                      rng.standard_normal((B, M, Ty)).astype(np.float32), logw, durations)


def malformed_durations(g):
    """The recipe of test_malformed_durations_are_clipped at two tokens per thread.  -> (all, only item 1's): item 0's counts run
    past Ty; item 1 holds a negative count and a count behind its x_mask, both in the second token of a thread's chunk."""
    assert scan_chunk(g["mu_x"].shape[2]) == 2
    only1 = g["durations"].copy()
    only1[1, 55] = -4
    only1[1, 201] = 7
    both = only1.copy()
    both[0, 130] += 400
    return both, only1


@functools.lru_cache(maxsize=None)
def restated(case_key, durations_key=None):
    """forward and backward of tests/align_loss_restatement.py on a case, once.  case_key: ("scan", shape), ("grid", (B, Tx)) or
    ("chain",); durations_key: None, "malformed" or "malformed1"."""
    g = case_by_key(case_key)
    dur = g["durations"]
    if durations_key is not None:
        dur = malformed_durations(g)[0 if durations_key == "malformed" else 1]
    f = ar.forward(g["mu_x64"], g["x_mask"], g["logw64"], g["x_lengths"], g["y64"], g["y_mask"], dur, g["keep"], g["fake_content64"])
    r = ar.backward(g["mu_x64"], g["x_mask"], g["logw64"], g["x_lengths"], g["y64"], g["y_mask"], dur, g["keep"], g_masked=g["W64"],
                    g_prior=1.0, g_dur=1.0)
    return f, r


def case_by_key(key):
    if key[0] == "scan":
        return scan_case(key[1])
    if key[0] == "grid":
        return duration_grid_case(*key[1])
    return aligned_case(CHAIN_SHAPE, CHAIN_ITEMS, 4999)


def zero_token_on_a_chunk_edge(g, durations=None):
    """Is some token without frames the first or the last token of a thread's chunk of the kernels' scan?"""
    Tx = g["mu_x"].shape[2]
    chunk = scan_chunk(Tx)
    ends = ar.segment_ends(g["durations"] if durations is None else durations, g["x_mask"], g["y"].shape[2])
    n = np.diff(ends, axis=1, prepend=0)
    j = np.arange(Tx)
    edge = (j % chunk == 0) | (j % chunk == chunk - 1) | (j == Tx - 1)
    return bool(((n == 0) & edge[None] & (j[None] < g["x_lengths"][:, None])).any())


# ---- length regulation past 256 tokens: (B, Tx, x_lengths, M, length_scale, seed) as oracle.make_golden_align.CASES; the seeds
# are the first ones at which no exp(logw) sits within 1e-5 (relative) of an integer (tests/test_align_sweep_cpu.py asserts it)
REGULATE_CASES = {
    "tx256": (2, 256, [256, 1], 80, 1.0, 11),
    "tx257": (2, 257, [257, 1], 16, 2.0, 12),
    "tx700": (3, 700, [700, 513, 1], 128, 0.5, 13),
}
