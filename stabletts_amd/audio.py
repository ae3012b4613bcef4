"""Drop-in replacement for the reference's ``utils/audio.py``: ``LinearSpectrogram``, ``LogMelSpectrogram`` and
``load_and_resample_audio`` (used by api.py:45,72-73, preprocess.py:50,73, vocoders/vocos/dataset.py:15,35 and the Vocos
loss).

Same constructors and module tree (``spectrogram.window``, ``mel_scale.fb``), so the ``state_dict()`` keys and shapes equal
the reference module's and ``LogMelSpectrogram(**asdict(MelConfig()))`` works unchanged.  The filter bank is built here
(``melscale_fbanks``, a restatement of torchaudio's formula), so nothing needs torchaudio; a loaded ``fb`` or ``window``
wins over the built ones.  The forward pass (reflect padding, window, real FFT, magnitude, banded mel projection, log) runs
in fp32 in libstabletts_hip.so behind ``st_mel_forward`` / ``st_mel_forward_ragged``; there is no PyTorch fallback, and it
runs on a HIP device only.

Gradients: these classes are inference-only (``native_training = False``): a grad-enabled call on a waveform that requires grad
raises.  The subclasses of ``stabletts_amd.audio_train`` (``install(audio="train")``, for the Vocos multi-scale mel loss) set
``native_training = True``: such a call runs the same forward kernel, and ``backward`` runs ``st_mel_backward`` (the spectrum
and mel sums recomputed, dmel, the transposed band projection, an inverse real FFT per frame and a deterministic overlap-add
gather), giving the waveform's gradient in its own shape and dtype.  There is no double backward, the window and the filter bank
get no gradient, and ``forward_ragged`` stays inference-only.

Native limits: ``center=False``, ``pad_mode="reflect"``, ``win_length == n_fft``, ``n_fft`` a power of two in [32, 2048].

Resampling: ``resample``, ``resample_ragged`` and ``Resample`` are ``torchaudio.functional.resample`` /
``torchaudio.transforms.Resample`` without torchaudio.  An fp32 waveform on a HIP device runs the polyphase filter in
libstabletts_hip.so (``st_resample``) through a compact tap table built here in float64 (only the taps inside the window: 14 per
phase at 48000 -> 44100 where the dense form has 174); CPU tensors, other dtypes and grad-enabled calls run the dense
formulation in torch (``F.pad`` + strided ``conv1d``), which is differentiable.  ``load_and_resample_wav`` decodes RIFF/WAVE PCM
with the standard library and resamples with ``resample``: file to log-mel needs no third-party library.  Other containers and
codecs (flac, mp3, float WAV) still need torchaudio: ``load_and_resample_audio`` imports it when called.
"""
import ctypes
import math
import wave

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._native_module import hip_device_index

_PAD_MODES = ("constant", "reflect", "replicate", "circular")


# ---------------------------------------------------------------- filter bank (torchaudio.functional.melscale_fbanks)
def _hz_to_mel(freq, mel_scale="htk"):
    if mel_scale not in ("slaney", "htk"):
        raise ValueError('mel_scale should be one of "htk" or "slaney".')
    if mel_scale == "htk":
        return 2595.0 * math.log10(1.0 + freq / 700.0)
    f_sp, min_log_hz = 200.0 / 3, 1000.0          # slaney: linear below 1 kHz, logarithmic above
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    if freq >= min_log_hz:
        return min_log_mel + math.log(freq / min_log_hz) / logstep
    return freq / f_sp


def _mel_to_hz(mels, mel_scale="htk"):
    if mel_scale not in ("slaney", "htk"):
        raise ValueError('mel_scale should be one of "htk" or "slaney".')
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (mels / 2595.0) - 1.0)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    freqs = f_sp * mels
    log_t = mels >= min_log_mel
    freqs[log_t] = min_log_hz * torch.exp(logstep * (mels[log_t] - min_log_mel))
    return freqs


def melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None, mel_scale="htk"):
    """(n_freqs, n_mels) triangular filter bank, fp32, as torchaudio.functional.melscale_fbanks computes it."""
    if norm is not None and norm != "slaney":
        raise ValueError('norm must be one of None or "slaney"')
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_pts = torch.linspace(_hz_to_mel(f_min, mel_scale), _hz_to_mel(f_max, mel_scale), n_mels + 2)
    f_pts = _mel_to_hz(m_pts, mel_scale)
    f_diff = f_pts[1:] - f_pts[:-1]                                   # (n_mels + 1)
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)              # (n_freqs, n_mels + 2)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.max(torch.zeros(1), torch.min(down, up))
    if norm == "slaney":
        fb *= (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])).unsqueeze(0)
    return fb


class MelScale(nn.Module):
    """torchaudio.transforms.MelScale's constructor and ``fb`` buffer (n_stft, n_mels); the projection itself runs inside the
    native LogMelSpectrogram."""

    def __init__(self, n_mels=128, sample_rate=16000, f_min=0.0, f_max=None, n_stft=201, norm=None, mel_scale="htk"):
        super().__init__()
        self.n_mels = n_mels
        self.sample_rate = sample_rate
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        self.f_min = f_min
        self.norm = norm
        self.mel_scale = mel_scale
        if f_min > self.f_max:
            raise ValueError(f"Require f_min: {f_min} <= f_max: {self.f_max}")
        self.register_buffer("fb", melscale_fbanks(n_stft, self.f_min, self.f_max, n_mels, sample_rate, norm, mel_scale))

    def forward(self, specgram):
        raise NotImplementedError("stabletts_amd: the mel projection runs inside the native LogMelSpectrogram")


# ---------------------------------------------------------------- native front end
def frames(L, n_fft, hop_length, pad):
    """Frames of an utterance of L samples with center=False: 1 + (L + 2 pad - n_fft) // hop.  Raises ValueError where the
    reference's reflect padding (pad < L) or torch.stft (at least one frame) would."""
    if L <= pad:
        raise ValueError(f"reflect padding of {pad} needs more than {pad} samples, got {L}")
    if L + 2 * pad < n_fft:
        raise ValueError(f"{L} samples padded by {pad} on both sides are shorter than n_fft = {n_fft}")
    return 1 + (L + 2 * pad - n_fft) // hop_length


def _check_config(n_fft, win_length, hop_length, pad, center, pad_mode):
    """Raises what the native kernels do not support (NotImplementedError) or what is invalid (ValueError), before any
    device is touched -- the checks of st_create_mel_extractor."""
    if n_fft < 1 or win_length < 1 or hop_length < 1 or pad < 0:
        raise ValueError("n_fft, win_length and hop_length must be positive and pad non-negative")
    if hop_length > n_fft:
        raise ValueError("hop_length must not exceed n_fft")
    if win_length > n_fft:
        raise ValueError("win_length must not exceed n_fft (torch.stft)")
    if pad_mode not in _PAD_MODES:
        raise ValueError(f"pad_mode must be one of {_PAD_MODES}")
    if center:
        raise NotImplementedError("native spectrogram kernels are built for center=False")
    if pad_mode != "reflect":
        raise NotImplementedError("native spectrogram kernels are built for pad_mode='reflect'")
    if win_length != n_fft:
        raise NotImplementedError("native spectrogram kernels are built for win_length == n_fft")
    if n_fft < 32 or n_fft > 2048 or n_fft & (n_fft - 1):
        raise NotImplementedError("native spectrogram kernels are built for n_fft a power of two in [32, 2048]")


def _version(t):
    """A tensor's version counter; inference tensors (a module built or moved under torch.inference_mode) have none and key on
    their address alone, so an in-place write to them needs sync_weights()."""
    try:
        return t._version
    except RuntimeError:
        return -1


class _Extractor:
    """One mel-extractor handle on the buffers' device, re-loaded when a buffer's storage or version counter changes (a
    ``load_state_dict``, ``.to()`` or an in-place write)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.engine = None
        self.key = None

    def __getstate__(self):
        return {"cfg": self.cfg, "engine": None, "key": None}

    def get(self, buffers):
        dev = hip_device_index(next(iter(buffers.values())).device, "spectrogram")
        if self.engine is None or self.engine.device != dev:
            if self.engine is not None:
                self.engine.close()
            self.engine = _lib.Engine(0, 0, 0, 0, 0, 0, 0, "f16", dev, mel=self.cfg)
            self.key = None
        key = tuple((n, t.data_ptr(), _version(t)) for n, t in buffers.items())
        if key != self.key:
            with torch.no_grad():
                torch.cuda.synchronize(dev)
                self.engine.load_state_dict(buffers)
            self.key = key
        return self.engine


def _waveform(x, dev, grad_ok=False):
    """(B, L) or (B, 1, L) -> (B, L) fp32 contiguous, with the module's device and gradient rules."""
    if not grad_ok and torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError("the native spectrogram is inference-only here (native_training = False, or a ragged batch): "
                                  "call it under torch.no_grad(), or use stabletts_amd.audio_train (install(audio=\"train\"))")
    hip_device_index(dev, "spectrogram")
    if x.device != dev:
        raise ValueError(f"the waveform is on {x.device}, the module's buffers are on {dev}")
    if x.dim() == 3:
        if x.shape[1] != 1:
            raise ValueError("a 3-d waveform must be (B, 1, L)")
        x = x.squeeze(1)
    if x.dim() != 2:
        raise ValueError("waveform must be (B, L) or (B, 1, L)")
    return x.detach().to(torch.float32).contiguous()


def _ragged(eng, waves, dev, rows, output, frames_of):
    """A list of 1-D waveforms -> a list of (rows, frames_b) results, in one launch."""
    ws = []
    for w in waves:
        w = _waveform(w.reshape(1, -1), dev)[0]
        ws.append(w)
    s_off, f_off = [0], [0]
    for w in ws:
        s_off.append(s_off[-1] + w.numel())
        f_off.append(f_off[-1] + frames_of(w.numel()))
    with torch.no_grad():
        wave = torch.cat(ws) if len(ws) > 1 else ws[0]
        out = torch.empty(rows * f_off[-1], device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            eng.mel_forward_ragged(wave, s_off, f_off, output, out, torch.cuda.current_stream(dev).cuda_stream)
    return [out[rows * f_off[b]:rows * f_off[b + 1]].view(rows, f_off[b + 1] - f_off[b]) for b in range(len(ws))]


def _wants_grad(module, x):
    return module.native_training and torch.is_grad_enabled() and x.requires_grad


class _SpectrogramFn(torch.autograd.Function):
    """The native forward under autograd; backward = st_mel_backward.  `run(wave)` is the module's forward on the (B, L) fp32
    waveform and `eng` the handle it ran on."""

    @staticmethod
    def forward(ctx, x, wave, eng, output, run):
        ctx.save_for_backward(wave)
        ctx.eng, ctx.output, ctx.shape, ctx.dtype = eng, output, x.shape, x.dtype
        return run(wave)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        (wave,) = ctx.saved_tensors
        B, L = wave.shape
        dev = wave.device
        g = grad.to(torch.float32).contiguous()
        gx = torch.empty(B, L, device=dev, dtype=torch.float32)
        ws = torch.empty(ctx.eng.mel_backward_workspace_bytes(B, L), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            ctx.eng.mel_backward(wave, g, ctx.output, gx, ws, torch.cuda.current_stream(dev).cuda_stream)
        return gx.view(ctx.shape).to(ctx.dtype), None, None, None, None


class LinearSpectrogram(nn.Module):
    """utils/audio.py:6-26: waveform (B, L) or (B, 1, L) -> magnitude (B, n_fft // 2 + 1, frames)."""

    native_training = False     # True (audio_train): differentiable in the waveform through st_mel_backward

    def __init__(self, n_fft, win_length, hop_length, pad, center, pad_mode):
        super().__init__()
        self.n_fft = n_fft
        self.win_length = win_length
        self.hop_length = hop_length
        self.pad = pad
        self.center = center
        self.pad_mode = pad_mode
        _check_config(n_fft, win_length, hop_length, pad, center, pad_mode)
        self.register_buffer("window", torch.hann_window(win_length))
        self._native = _Extractor(dict(n_fft=n_fft, win_length=win_length, hop_length=hop_length, pad=pad, n_mels=0,
                                       center=0, pad_mode=_lib.ST_PAD_MODES[pad_mode]))

    def frames(self, L):
        return frames(L, self.n_fft, self.hop_length, self.pad)

    def sync_weights(self):
        """Force a re-read of the window at the next call (after writes that bypass the version counter)."""
        self._native.key = None

    def _engine(self):
        return self._native.get({"spectrogram.window": self.window})

    def forward(self, waveform):
        grad = _wants_grad(self, waveform)
        wave = _waveform(waveform, self.window.device, grad)
        eng = self._engine()
        if grad:
            return _SpectrogramFn.apply(waveform, wave, eng, _lib.ST_MEL_LINEAR, lambda w: self._run(eng, w))
        return self._run(eng, wave)

    def _run(self, eng, wave):
        B, L = wave.shape
        bins, T = self.n_fft // 2 + 1, self.frames(L)
        out = torch.empty(B * bins * T, device=wave.device, dtype=torch.float32)
        dev = wave.device
        with torch.cuda.device(dev):
            eng.mel_forward_ragged(wave, [b * L for b in range(B + 1)], [b * T for b in range(B + 1)], _lib.ST_MEL_LINEAR, out,
                                   torch.cuda.current_stream(dev).cuda_stream)
        return out.view(B, bins, T)

    def forward_ragged(self, waves):
        """A list of 1-D waveforms of any lengths -> a list of (n_fft // 2 + 1, frames_b) magnitudes, in one launch."""
        eng = self._engine()
        return _ragged(eng, waves, self.window.device, self.n_fft // 2 + 1, _lib.ST_MEL_LINEAR, self.frames)


class LogMelSpectrogram(nn.Module):
    """utils/audio.py:29-52: waveform (B, L) or (B, 1, L) -> log-mel (B, n_mels, frames)."""

    native_training = False     # True (audio_train): differentiable in the waveform through st_mel_backward

    def __init__(self, sample_rate, n_fft, win_length, hop_length, f_min, f_max, pad, n_mels, center, pad_mode, mel_scale):
        super().__init__()
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.win_length = win_length
        self.hop_length = hop_length
        self.f_min = f_min
        self.f_max = f_max
        self.pad = pad
        self.n_mels = n_mels
        self.center = center
        self.pad_mode = pad_mode
        if n_mels < 1:
            raise ValueError("n_mels must be positive")
        self.spectrogram = LinearSpectrogram(n_fft, win_length, hop_length, pad, center, pad_mode)
        # called as utils/audio.py:45 calls torchaudio.transforms.MelScale: mel_scale is both norm and mel_scale
        self.mel_scale = MelScale(n_mels, sample_rate, f_min, f_max, (n_fft // 2) + 1, mel_scale, mel_scale)
        self._native = _Extractor(dict(n_fft=n_fft, win_length=win_length, hop_length=hop_length, pad=pad, n_mels=n_mels,
                                       center=0, pad_mode=_lib.ST_PAD_MODES[pad_mode]))

    def compress(self, x):
        return torch.log(torch.clamp(x, min=1e-5))

    def decompress(self, x):
        return torch.exp(x)

    def frames(self, L):
        return frames(L, self.n_fft, self.hop_length, self.pad)

    def sync_weights(self):
        """Force a re-read of the window and the filter bank at the next call (after writes that bypass the version counter)."""
        self._native.key = None

    def _engine(self):
        return self._native.get({"spectrogram.window": self.spectrogram.window, "mel_scale.fb": self.mel_scale.fb})

    def forward(self, x):
        grad = _wants_grad(self, x)
        wave = _waveform(x, self.spectrogram.window.device, grad)
        if self.mel_scale.fb.device != wave.device:
            raise ValueError("spectrogram.window and mel_scale.fb are on different devices")
        eng = self._engine()
        if grad:
            return _SpectrogramFn.apply(x, wave, eng, _lib.ST_MEL_LOG, lambda w: self._run(eng, w))
        return self._run(eng, wave)

    def _run(self, eng, wave):
        B, L = wave.shape
        dev = wave.device
        out = torch.empty(B, self.n_mels, self.frames(L), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            eng.mel_forward(wave, out, torch.cuda.current_stream(dev).cuda_stream)
        return out

    def forward_ragged(self, waves):
        """A list of 1-D waveforms of any lengths -> a list of (n_mels, frames_b) log-mels, in one launch; each equals the
        utterance run alone, bit for bit."""
        eng = self._engine()
        return _ragged(eng, waves, self.spectrogram.window.device, self.n_mels, _lib.ST_MEL_LOG, self.frames)


def load_and_resample_audio(audio_path, target_sr, device="cpu"):
    """utils/audio.py:54-70: (1, time) mono waveform at target_sr, or None when the file cannot be read.  Decoding and
    resampling are torchaudio's; it is imported here, so the rest of this module needs no torchaudio."""
    try:
        import torchaudio
    except ImportError as e:
        raise ImportError("load_and_resample_audio needs torchaudio (audio file decoding and resampling are not native); "
                          "LogMelSpectrogram itself does not") from e
    try:
        y, sr = torchaudio.load(audio_path)
    except Exception as e:      # the reference reports the failure and returns None (preprocess.py:64 skips the file)
        print(str(e))
        return None
    if y.size(0) > 1:           # first channel only
        y = y[0, :].unsqueeze(0)
    if sr != target_sr:
        y = torchaudio.functional.resample(y, sr, target_sr)
    return y


# ---------------------------------------------------------------- resampling (torchaudio.functional.resample)
_RESAMPLING_METHODS = ("sinc_interp_hann", "sinc_interp_kaiser")
_KAISER_BETA = 14.769656459379492
RESAMPLE_MAX_TABLE = 1 << 22        # new * S entries of a compact table (st_resample's limit: 16 MB, 32-bit tap indices)
_filters = {}                       # (key, "dense" | "compact", device, dtype) -> the cached filter


def _resample_key(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta):
    """The checked arguments as the cache key (orig, new, lowpass_filter_width, rolloff, method, beta), rates divided by
    their greatest common divisor."""
    for name, v in (("orig_freq", orig_freq), ("new_freq", new_freq)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v:
            raise ValueError(f"{name} must be an integer sample rate, got {v!r} (torchaudio: frequencies must be of integer type "
                             "to ensure quality resampling computation)")
        if v <= 0:
            raise ValueError(f"{name} must be positive, got {v!r}")
    if lowpass_filter_width <= 0:
        raise ValueError("Low pass filter width should be positive.")
    if not rolloff > 0:
        raise ValueError("rolloff must be positive")
    if resampling_method not in _RESAMPLING_METHODS:
        raise ValueError(f"Invalid resampling method: {resampling_method}")
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    g = math.gcd(orig_freq, new_freq)
    if resampling_method == "sinc_interp_hann":
        beta = None
    else:
        beta = _KAISER_BETA if beta is None else float(beta)
    return (orig_freq // g, new_freq // g, lowpass_filter_width, float(rolloff), resampling_method, beta)


def _sinc_taps(t, lowpass_filter_width, method, beta, scale):
    """The filter at the float64 times t (in periods of the cut-off, unclamped), in torchaudio's order of operations."""
    t = t.clamp(-lowpass_filter_width, lowpass_filter_width)
    if method == "sinc_interp_hann":
        window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    else:
        beta_t = torch.tensor(beta, dtype=torch.float64)
        window = torch.i0(beta_t * torch.sqrt(1 - (t / lowpass_filter_width) ** 2)) / torch.i0(beta_t)
    t = t * math.pi
    taps = torch.where(t == 0, torch.ones((), dtype=torch.float64), t.sin() / t)
    return taps * (window * scale)


def _filter_geometry(key):
    orig, new, lpw, rolloff = key[:4]
    base = min(orig, new) * rolloff
    return base, math.ceil(lpw * orig / base), base / orig


def _dense_kernel(key, device, dtype):
    """torchaudio's kernel (new, 1, 2 width + orig) built in float64 on the device and rounded once to dtype, and width."""
    hit = _filters.get((key, "dense", device, dtype))
    if hit is None:
        orig, new, lpw, _, method, beta = key
        base, width, scale = _filter_geometry(key)
        idx = torch.arange(-width, width + orig, dtype=torch.float64, device=device)[None, None] / orig
        t = torch.arange(0, -new, -1, dtype=torch.float64, device=device)[:, None, None] / new + idx
        t *= base
        hit = _filters[(key, "dense", device, dtype)] = (_sinc_taps(t, lpw, method, beta, scale).to(dtype), width)
    return hit


def _compact_table(key, device):
    """The compact form of the dense kernel: of phase i only the taps with |t| < lowpass_filter_width (the others are zero in fp32
    for the Hann window and below 2^-60 of the scale for Kaiser's), which are contiguous.  -> (taps (S, new) fp32 tap-major,
    first (new) int32: the offset of a phase's first tap from j * orig, S).  Only the band is evaluated, in float64 and in the
    dense kernel's order of operations, so a kept tap is the dense entry bit for bit."""
    hit = _filters.get((key, "compact", device, None))
    if hit is not None:
        return hit
    cpu = torch.device("cpu")
    hit = _filters.get((key, "compact", cpu, None))
    if hit is None:
        orig, new, lpw, _, method, beta = key
        base, width, scale = _filter_geometry(key)
        half = lpw * orig / base                    # a phase keeps the offsets o with |o - i orig / new| < half
        limit = f"the native resampler's tap table is limited to new * S <= 2^22 entries (RESAMPLE_MAX_TABLE), {orig} -> {new} needs "
        if new * (math.ceil(2 * half) - 1) > RESAMPLE_MAX_TABLE:
            raise NotImplementedError(limit + f"at least {new * (math.ceil(2 * half) - 1)}")
        n_cand = 2 * math.ceil(half) + 4
        phase = torch.arange(new, dtype=torch.int64)
        start = (phase * orig) // new - math.ceil(half) - 1
        o = start[:, None] + torch.arange(n_cand, dtype=torch.int64)[None]
        t = (-phase).to(torch.float64)[:, None] / new + o.to(torch.float64) / orig
        t *= base
        kept = (t.abs() < lpw) & (o >= -width) & (o < width + orig)
        count = kept.sum(1)
        k0 = kept.to(torch.int32).argmax(1)
        k1 = n_cand - 1 - kept.flip(1).to(torch.int32).argmax(1)
        assert bool((count >= 1).all()) and bool((k1 - k0 + 1 == count).all()), "a phase's kept taps are contiguous"
        S = int(count.max())
        if new * S > RESAMPLE_MAX_TABLE:
            raise NotImplementedError(limit + f"{new * S}")
        s = torch.arange(S, dtype=torch.int64)[None]
        vals = _sinc_taps(t, lpw, method, beta, scale).gather(1, (k0[:, None] + s).clamp(max=n_cand - 1)).to(torch.float32)
        taps = torch.where(s < count[:, None], vals, torch.zeros((), dtype=torch.float32)).t().contiguous()
        hit = _filters[(key, "compact", cpu, None)] = (taps, (start + k0).to(torch.int32), S)
    if device != cpu:
        hit = _filters[(key, "compact", device, None)] = (hit[0].to(device), hit[1].to(device), hit[2])
    return hit


def resample_table(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None,
                   device="cpu"):
    """The compact tap table st_resample reads, cached per (rates, filter arguments, device): dict(taps (S, new) fp32,
    first (new) int32, S, orig, new, width).  NotImplementedError where new * S exceeds RESAMPLE_MAX_TABLE."""
    key = _resample_key(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
    taps, first, S = _compact_table(key, torch.device(device))
    return dict(taps=taps, first=first, S=S, orig=key[0], new=key[1], width=_filter_geometry(key)[1])


def _out_len(L, orig, new):
    return -((-new * L) // orig)


def _native_waveform(w):
    return w.is_cuda and w.dtype is torch.float32 and not (torch.is_grad_enabled() and w.requires_grad)


def _resample_dense(waveform, key):
    """torchaudio's formulation in torch: the dense kernel in the waveform's dtype, F.pad and a strided conv1d."""
    if not waveform.is_floating_point():
        raise TypeError(f"Expected floating point type for waveform tensor, but received {waveform.dtype}.")
    orig, new = key[:2]
    kernel, width = _dense_kernel(key, waveform.device, waveform.dtype)
    shape = waveform.shape
    L = shape[-1]
    x = F.pad(waveform.reshape(-1, L), (width, width + orig))
    y = F.conv1d(x[:, None], kernel, stride=orig).transpose(1, 2).reshape(x.shape[0], -1)[..., :_out_len(L, orig, new)]
    return y.reshape(shape[:-1] + y.shape[-1:])


def _resample_native(key, xs, ys):
    """xs, ys: fp32 1-D contiguous views on one HIP device, ys[b] of _out_len(xs[b]) samples -- one st_resample call."""
    rows = [(x.data_ptr(), y.data_ptr(), x.numel(), y.numel()) for x, y in zip(xs, ys) if x.numel() > 0]
    if not rows:
        return
    dev = xs[0].device
    taps, first, S = _compact_table(key, dev)
    n = len(rows)
    cols = list(zip(*rows))
    ptr_t, i64_t = ctypes.c_void_p * n, ctypes.c_int64 * n
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.st_resample(ptr_t(*cols[0]), ptr_t(*cols[1]), i64_t(*cols[2]), i64_t(*cols[3]), n, key[0], key[1],
                             taps.data_ptr(), first.data_ptr(), S, stream)
    if rc != _lib.ST_OK:
        raise _lib.NativeError(rc, lib.st_last_error(None).decode())


def _resample(waveform, key):
    orig, new = key[:2]
    if orig == new:
        return waveform
    shape = waveform.shape
    L = shape[-1]
    if waveform.numel() == 0:
        return waveform.new_empty(shape[:-1] + (_out_len(L, orig, new),))
    if not _native_waveform(waveform):
        return _resample_dense(waveform, key)
    x = waveform.detach().reshape(-1, L).contiguous()
    y = torch.empty(x.shape[0], _out_len(L, orig, new), device=x.device, dtype=torch.float32)
    _resample_native(key, list(x), list(y))
    return y.view(shape[:-1] + y.shape[-1:])


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """``torchaudio.functional.resample``: waveform (..., L) at orig_freq -> (..., ceil(new L / orig)) at new_freq, with the
    rates divided by their greatest common divisor.  An fp32 tensor on a HIP device runs natively (``st_resample``) unless it
    requires grad with autograd enabled; anything else -- CPU tensors, other dtypes, grad-enabled calls -- runs torchaudio's
    dense formulation in torch, differentiably.  Equal rates return the waveform itself."""
    return _resample(waveform, _resample_key(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta))


def resample_ragged(waves, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """A list of 1-D waveforms of any lengths -> the list of their resampled waveforms, each bit for bit the one ``resample``
    gives for it alone.  fp32 waveforms on one HIP device run as ONE native call without concatenation (64 waveforms per
    launch; the results are views of one buffer); any other list is ``resample`` per waveform."""
    key = _resample_key(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
    waves = list(waves)
    for w in waves:
        if w.dim() != 1:
            raise ValueError("resample_ragged takes 1-D waveforms")
    orig, new = key[:2]
    if orig == new:
        return waves
    if not waves or not all(_native_waveform(w) and w.device == waves[0].device for w in waves):
        return [_resample(w, key) for w in waves]
    xs = [w.detach().contiguous() for w in waves]
    lens = [_out_len(x.numel(), orig, new) for x in xs]
    ys = list(torch.empty(sum(lens), device=xs[0].device, dtype=torch.float32).split(lens))
    _resample_native(key, xs, ys)
    return ys


class Resample(nn.Module):
    """``torchaudio.transforms.Resample``: the constructor's filter applied by ``resample``.  The filter tables are built at the
    first call on a device and cached there; like torchaudio's non-persistent ``kernel`` buffer they are no ``state_dict()``
    entry."""

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99,
                 beta=None):
        super().__init__()
        self._key = _resample_key(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
        self.orig_freq = orig_freq
        self.new_freq = new_freq
        self.gcd = math.gcd(int(orig_freq), int(new_freq))
        self.resampling_method = resampling_method
        self.lowpass_filter_width = lowpass_filter_width
        self.rolloff = rolloff
        self.beta = beta

    def forward(self, waveform):
        return _resample(waveform, self._key)

    def forward_ragged(self, waves):
        """``resample_ragged`` with the constructor's filter."""
        k = self._key
        return resample_ragged(waves, self.orig_freq, self.new_freq, k[2], k[3], k[4], k[5])


def _decode_wav(audio_path):
    """RIFF/WAVE PCM through the standard library -> ((channels, frames) fp32 in [-1, 1), sample rate): 8-bit unsigned as
    (v - 128) / 128, 16-, 24- and 32-bit signed as v / 2^(bits - 1)."""
    with wave.open(audio_path, "rb") as f:          # wave.Error for anything but PCM (format tag 1)
        channels, width, rate, frames = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        raw = f.readframes(frames)
    if width not in (1, 2, 3, 4):
        raise ValueError(f"unsupported sample width of {width} bytes")
    raw = raw[:len(raw) - len(raw) % (width * channels)]
    if not raw:
        return torch.zeros(channels, 0), rate
    b = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    if width == 1:
        v = b.to(torch.float64) - 128.0
    elif width == 2:
        v = b.view(torch.int16).to(torch.float64)    # RIFF is little-endian, as every host this runs on
    elif width == 4:
        v = b.view(torch.int32).to(torch.float64)
    else:
        b = b.view(-1, 3).to(torch.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = ((v ^ 0x800000) - 0x800000).to(torch.float64)            # sign extension of the 24-bit value
    v = (v / float(1 << (8 * width - 1))).to(torch.float32)
    return v.view(-1, channels).t().contiguous(), rate


def load_and_resample_wav(audio_path, target_sr, device="cpu"):
    """The reference's ``load_and_resample_audio`` (utils/audio.py:59-74) for RIFF/WAVE PCM files without torchaudio: the first
    channel as a (1, time) fp32 waveform at target_sr, or None -- with the error printed -- when the file cannot be read
    (missing, not a WAVE file, not PCM).  Decoding is the standard library's ``wave``; resampling is ``resample`` ON
    ``device``, natively where that is a HIP device.  Unlike the reference, whose ``y.to(device)`` discards its result and
    returns a CPU tensor whatever ``device`` is, the waveform returned here is on ``device``."""
    try:
        y, sr = _decode_wav(audio_path)
    except Exception as e:      # the reference reports the failure and returns None (preprocess.py:64 skips the file)
        print(str(e))
        return None
    y = y[:1].to(device)        # first channel only
    if sr != target_sr:
        y = resample(y, sr, target_sr)
    return y
