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
File decoding and resampling still need torchaudio (``load_and_resample_audio`` imports it when called).
"""
import math

import torch
import torch.nn as nn

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
