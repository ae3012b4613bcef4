"""float64 restatements of torchaudio.functional.resample for the resampler's tests, written from the formula alone:

    g = gcd(orig_freq, new_freq); orig, new = orig_freq / g, new_freq / g
    base = min(orig, new) rolloff; width = ceil(lowpass_filter_width orig / base); scale = base / orig
    K[i][m] = scale sinc(pi tc) window(tc),  tc = clamp(base ((m - width) / orig - i / new), +-lowpass_filter_width)
    y[j new + i] = sum_m K[i][m] x[j orig + m - width],  x zero outside [0, L),  for j new + i < ceil(new L / orig)

``dense`` is that sum as a padded, strided conv1d over the whole (new, 2 width + orig) kernel, evaluated a block of phases at a
time (at 8000 -> 44101 the kernel has 353 M entries); ``direct`` is an independent gather-sum over the kept band of each phase
(|t| < lowpass_filter_width, t unclamped), without conv1d and without the dense kernel.  Both sum in float64 and take the taps
rounded once to ``taps`` first: fp32 by default, as every fp32 implementation under test stores them, float64 (no rounding) for a
float64 waveform, whose kernel torchaudio keeps in float64."""
import math

import torch

KAISER_BETA = 14.769656459379492
KAISER = dict(lowpass_filter_width=64, rolloff=0.9475937167399596, resampling_method="sinc_interp_kaiser")
# (orig_freq, new_freq, filter arguments): the nine configurations of the issue
CONFIGS = [(22050, 44100, {}), (44100, 22050, {}), (48000, 44100, {}), (16000, 44100, {}), (44100, 16000, {}), (24000, 44100, {}),
           (8000, 44101, {}), (48000, 44100, KAISER), (44100, 16000, KAISER)]
IDS = [f"{o}-{n}" + ("-kaiser" if kw else "") for o, n, kw in CONFIGS]
S_EXPECTED = {"48000-44100": 14, "44100-16000": 34, "44100-16000-kaiser": 373}
PHASE_BLOCK = 2048          # phases of the dense kernel evaluated at a time


def geometry(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, **_):
    """-> orig, new, base, width, scale"""
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * rolloff
    return orig, new, base, math.ceil(lowpass_filter_width * orig / base), base / orig


def kernel_at(t, scale, lowpass_filter_width=6, resampling_method="sinc_interp_hann", beta=None, **_):
    """scale sinc(pi tc) window(tc) at the unclamped float64 times t"""
    lpw = lowpass_filter_width
    t = t.clamp(-lpw, lpw)
    if resampling_method == "sinc_interp_hann":
        window = torch.cos(t * math.pi / lpw / 2) ** 2
    else:
        b = torch.tensor(KAISER_BETA if beta is None else float(beta), dtype=torch.float64)
        window = torch.i0(b * torch.sqrt(1 - (t / lpw) ** 2)) / torch.i0(b)
    t = t * math.pi
    k = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t)
    k *= window * scale
    return k


def times(orig_freq, new_freq, phases=None, **kw):
    """t[i][m] = base ((m - width) / orig - i / new), unclamped, float64 (phases, 2 width + orig); phases: a (lo, hi) range"""
    orig, new, base, width, _ = geometry(orig_freq, new_freq, **kw)
    lo, hi = phases if phases is not None else (0, new)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None] / orig
    t = -torch.arange(lo, hi, dtype=torch.float64)[:, None] / new + idx
    t *= base
    return t


def dense_kernel(orig_freq, new_freq, phases=None, **kw):
    """K (phases, 2 width + orig) in float64"""
    return kernel_at(times(orig_freq, new_freq, phases, **kw), geometry(orig_freq, new_freq, **kw)[4], **kw)


def out_len(L, orig, new):
    return -((-new * L) // orig)


def dense(xs, orig_freq, new_freq, taps=torch.float32, **kw):
    """x (..., L) -> (..., ceil(new L / orig)) float64, or a list of such for a list: the dense kernel, zero padding and a
    strided conv1d.  The kernel is evaluated once for the whole list, PHASE_BLOCK phases at a time, and only as far as the
    longest output needs it."""
    orig, new, _, width, _ = geometry(orig_freq, new_freq, **kw)
    many = isinstance(xs, (list, tuple))
    work = []
    for x in (xs if many else [xs]):
        L = x.shape[-1]
        xp = torch.nn.functional.pad(x.double().reshape(-1, L), (width, width + orig))
        work.append((x.shape, xp, torch.zeros(xp.shape[0], L // orig + 1, new, dtype=torch.float64), out_len(L, orig, new)))
    for lo in range(0, min(new, max(w[3] for w in work)), PHASE_BLOCK):
        hi = min(new, lo + PHASE_BLOCK)
        k = dense_kernel(orig_freq, new_freq, (lo, hi), **kw).to(taps).double()
        for _, xp, y, n_out in work:
            if lo < n_out:
                y[:, :, lo:hi] = torch.nn.functional.conv1d(xp[:, None], k[:, None], stride=orig).transpose(1, 2)
    out = [y.reshape(y.shape[0], -1)[:, :n_out].reshape(shape[:-1] + (n_out,)) for shape, _, y, n_out in work]
    return out if many else out[0]


def band(t, lowpass_filter_width=6, **_):
    """The kept band of rows of times -> (keep mask, first kept m, kept count, whether every row's kept entries are contiguous)"""
    keep = t.abs() < lowpass_filter_width
    first, count = keep.to(torch.int32).argmax(1), keep.sum(1)
    last = keep.shape[1] - 1 - keep.flip(1).to(torch.int32).argmax(1)
    return keep, first, count, bool((last - first + 1 == count).all())


def direct(x, orig_freq, new_freq, taps=torch.float32, **kw):
    """x (L,) -> (ceil(new L / orig),) float64: per output sample, the products of its phase's kept taps with the samples inside
    [0, L), gathered by index and summed -- no conv1d, no padding, no dense kernel: the taps are evaluated on the offsets
    within width + 1 of each phase's centre i orig / new only."""
    orig, new, base, width, scale = geometry(orig_freq, new_freq, **kw)
    lpw = kw.get("lowpass_filter_width", 6)
    i = torch.arange(new)
    o = ((i * orig + new // 2) // new)[:, None] + torch.arange(-width - 1, width + 2)[None]        # offsets from j orig
    t = base * (o.double() / orig - i.double()[:, None] / new)
    keep = (t.abs() < lpw) & (o >= -width) & (o < width + orig)
    k = kernel_at(t, scale, **kw).to(taps).double() * keep
    L = x.numel()
    n_out = out_len(L, orig, new)
    x = x.double()
    y = torch.empty(n_out, dtype=torch.float64)
    for q0 in range(0, n_out, 8192):
        q = torch.arange(q0, min(n_out, q0 + 8192))
        j, ph = q // new, q % new
        p = (j * orig)[:, None] + o[ph]
        inside = (p >= 0) & (p < L)
        y[q0:q0 + q.numel()] = (k[ph] * torch.where(inside, x[p.clamp(0, max(L - 1, 0))], torch.zeros((), dtype=torch.float64))).sum(1)
    return y
