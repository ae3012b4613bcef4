"""Cases and checks of the spectrogram front end off the hop = n_fft / 4 lattice, shared by test_gpu_mel_sweep.py (the kernels
against float64) and test_mel_backward_cpu.py (the float64 restatement's own index inversion at the same cases).

A case is (n_fft, hop, pad, n_mels) at a frame count T.  With S = 2048 / n_fft frames per FFT round and FR = max(S, 8) frames per
block, T runs over {1 (or the smallest the configuration allows), S + 1, FR + 1, 2 FR + 1}; L is the largest length with that T,
(T - 1) hop + n_fft - 2 pad + hop - 1, raised to max(pad + 1, n_fft - 2 pad) where the reflect padding or the first frame needs it.

Accuracy bar: 4 x torch fp32's own distance from float64 (mv.torch_forward and its autograd on the CPU) on the same case and
metric -- the project's bar for fp32 kernels against float64.  Metrics: max abs for the log-mel, max abs / max |ref| for the
magnitude and for dx.  A maximum over a few hundred elements is a noisy yardstick: where a case misses 4 x its own, it is held to
4 x the largest yardstick of its family (the cases of the same n_fft, window, output and metric) -- the same factor over a less
noisy estimate of the same rounding error -- and reported as pooled.
"""
import functools

import numpy as np
import torch

from tests import mel_restatement as mr
from tests import mel_vjp_restatement as mv

SR = 44100
FLOOR = 1e-5
CONFIGS = [
    (32, 1, 0, 5),                  # hop 1, no reflection, up to 32 frames per sample in the gather
    (32, 32, 0, 64),                # no overlap, n_mels = 2 n_fft, 39 empty slaney filters
    (64, 7, 50, 10),                # odd hop, pad > hop, pad not (n_fft - hop) / 2
    (128, 100, 3, 20),              # 96 tail samples that no frame reads
    (256, 64, 255, 40),             # pad = n_fft - 1, first L = pad + 1: a sample read directly and by both reflections
    (512, 129, 0, 80),              # two FFT rounds per tile, the backward's early break
    (1024, 1024, 512, 160),         # no overlap with reflections
    (2048, 300, 1000, 320),
    (2048, 512, 768, 4096),         # n_mels = 2 n_fft at the largest FFT, 2385 empty filters
]
T_LIMIT = {(2048, 512, 768, 4096): 9}                       # the float64 side: 1.6 s at T = 9, 3.1 s at T = 17
HANN_CONFIGS = [(32, 1, 0, 5), (64, 7, 50, 10), (128, 100, 3, 20), (256, 64, 255, 40), (512, 129, 0, 80), (1024, 1024, 512, 160),
                (2048, 300, 1000, 320)]                     # one per n_fft, run with the periodic hann window as well


def tile(n_fft):
    """(frames per FFT round, frames per block) of the n_fft kernels."""
    S = 2048 // n_fft
    return S, max(S, 8)


def length_for(T, n_fft, hop, pad):
    return max((T - 1) * hop + n_fft - 2 * pad + hop - 1, pad + 1, n_fft - 2 * pad)


def frame_counts(cfg):
    """[(T, L)] of a configuration, ascending and distinct (a raised L gives the smallest T the configuration allows)."""
    n_fft, hop, pad, _ = cfg
    S, FR = tile(n_fft)
    out = {}
    for T in (1, S + 1, FR + 1, 2 * FR + 1):
        L = length_for(T, n_fft, hop, pad)
        T = mr.frames(L, n_fft, hop, pad)
        if T <= T_LIMIT.get(cfg, T):
            out[T] = L
    return sorted(out.items())


GEOMETRIES = sorted({(c[0], c[1], c[2], T, L) for c in CONFIGS for T, L in frame_counts(c)})       # (n_fft, hop, pad, T, L)
SWEEP = [(cfg, T, L, "uniform") for cfg in CONFIGS for T, L in frame_counts(cfg)] + \
        [(cfg, T, L, "hann") for cfg in HANN_CONFIGS for T, L in frame_counts(cfg)]


def case_id(case):
    (n_fft, hop, pad, n_mels), T, L, kind = case
    return f"{n_fft}-{hop}-{pad}-{n_mels}-T{T}-{kind}"


def window(n_fft, kind="uniform"):
    """"uniform": uniform(0.5, 1.5), asymmetric with non-zero ends; "hann": the module's own periodic hann window."""
    if kind == "hann":
        return torch.hann_window(n_fft).numpy()
    return np.random.Generator(np.random.PCG64(7000 + n_fft)).uniform(0.5, 1.5, n_fft).astype(np.float32)


def slaney(n_fft, n_mels):
    from stabletts_amd.audio import melscale_fbanks
    return melscale_fbanks(n_fft // 2 + 1, 0.0, float(SR // 2), n_mels, SR, "slaney", "slaney").numpy()


def waves(B, L, seed):
    return (0.3 * np.random.Generator(np.random.PCG64(seed)).standard_normal((B, L))).astype(np.float32)


def case_seed(case):
    (n_fft, hop, pad, n_mels), T, L, kind = case
    return (n_fft * 1000003 + hop * 10007 + pad * 101 + n_mels * 13 + T) % (1 << 31)


def rel_max(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def abs_max(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max())


METRIC = {"log-mel": abs_max, "linear": rel_max}


def reference(wave, win, fb, n_fft, hop, pad, seed):
    """Float64 and the torch fp32 yardstick of one call: {"log-mel" (when fb is given), "linear"} -> dict(y, g, dx, yard_y, yard_dx,
    zeroed).  g = standard_normal in fp32, zeroed where the float64 mel is within 1e-3 relative of the 1e-5 floor (a clamp-mask
    flip there is a property of fp32, not of a kernel)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mag = mr.linear(wave, win, n_fft, hop, pad)
    out = {}
    for kind, bank in (("log-mel", fb), ("linear", None)):
        if kind == "log-mel" and fb is None:
            continue
        if bank is not None:
            mel = np.einsum("km,bkt->bmt", bank.astype(np.float64), mag)
            y, near = np.log(np.maximum(mel, FLOOR)), np.abs(mel - FLOOR) <= 1e-3 * FLOOR
        else:
            y, near = mag, np.zeros(mag.shape, bool)
        g = rng.standard_normal(y.shape)
        g[near] = 0.0
        g = g.astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):                    # an empty filter: g / 0 under the mask
            dx = mv.vjp(wave, win, bank, n_fft, hop, pad, g)
        with torch.enable_grad():
            xt = torch.from_numpy(wave).requires_grad_(True)
            yt = mv.torch_forward(xt, torch.from_numpy(win), None if bank is None else torch.from_numpy(bank), n_fft, hop, pad)
            (dt,) = torch.autograd.grad(yt, xt, torch.from_numpy(g))
        out[kind] = dict(y=y, g=g, dx=dx, zeroed=int(near.sum()), yard_y=METRIC[kind](yt.detach().numpy(), y),
                         yard_dx=rel_max(dt.numpy(), dx))
    return out


@functools.lru_cache(maxsize=None)
def sweep_inputs(case):
    (n_fft, hop, pad, n_mels), T, L, kind = case
    return waves(2, L, case_seed(case)), window(n_fft, kind), slaney(n_fft, n_mels)


@functools.lru_cache(maxsize=None)
def sweep_reference(case):
    """reference() of a sweep case, computed once and shared (the pooled bars read the yardsticks of a case's whole family)."""
    (n_fft, hop, pad, n_mels), T, L, kind = case
    wave, win, fb = sweep_inputs(case)
    return reference(wave, win, fb, n_fft, hop, pad, case_seed(case) + 1)


def pooled_yardstick(case, kind, which):
    """The largest yardstick of the case's family: the sweep cases of the same n_fft and window, same output and metric."""
    return max(sweep_reference(c)[kind][which] for c in SWEEP if c[0][0] == case[0][0] and c[3] == case[3])


class Report:
    """Errors beside their bars: held(err, own, pooled_fn) says whether err <= 4 x own, or else <= 4 x the pooled yardstick."""

    def __init__(self):
        self.lines, self.pooled, self.fails, self.worst = [], [], [], (0.0, None)

    def held(self, name, err, own, pooled_fn=None):
        yard, note = own, ""
        if err > 4 * own and pooled_fn is not None:
            yard, note = max(own, pooled_fn()), " [pooled]"
            self.pooled.append(name)
        ratio = err / max(yard, 1e-30)
        line = f"{name}: native {err:.2e}, torch fp32 {own:.2e}, ratio {err / max(own, 1e-30):.2f}" + \
               (f", pooled yardstick {yard:.2e}, ratio {ratio:.2f}" if note else "") + f" (bar {4 * yard:.2e})"
        print(line)
        self.lines.append(line)
        self.worst = max(self.worst, (ratio, name))
        if not err <= 4 * yard:
            self.fails.append(line)
        return err <= 4 * yard


def two_lobe_bank(bins, n_mels, seed):
    """Filters of two disjoint positive lobes with zeros between them (and around them)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fb = np.zeros((bins, n_mels), np.float32)
    w = max(2, bins // 16)
    for m in range(n_mels):
        a = (m * 3) % (bins - 3 * w - 2)
        c = a + 2 * w + 1 + (m % 2)
        fb[a:a + w, m] = rng.uniform(0.2, 1.0, w) / w
        fb[c:c + w, m] = rng.uniform(0.2, 1.0, min(w, bins - c)) / w
    return fb


def banks(n_fft, n_mels, seed):
    """Filter banks the slaney construction never makes: name -> (bins, n_mels) fp32."""
    bins = n_fft // 2 + 1
    rng = np.random.Generator(np.random.PCG64(seed))
    base = slaney(n_fft, n_mels) * rng.uniform(0.5, 1.5, (bins, n_mels)).astype(np.float32)
    col3, rows = base.copy(), base.copy()
    col3[:, 3] = 0.0
    rows[0] = 0.0
    rows[bins - 1] = 0.0
    return {"dense": (rng.uniform(0.0, 1.0, (bins, n_mels)) / bins).astype(np.float32), "two_lobes": two_lobe_bank(bins, n_mels, seed + 1),
            "column3_zero": col3, "edge_rows_zero": rows}


def readers(s, L, T, n_fft, hop, pad):
    """The frames whose padded window reads sample s, directly or by a reflection: the index map itself, no inversion."""
    q = np.arange(T)[:, None] * hop + np.arange(n_fft)[None] - pad
    q = np.where(q < 0, -q, q)
    q = np.where(q >= L, 2 * (L - 1) - q, q)
    return np.nonzero((q == s).any(1))[0]
