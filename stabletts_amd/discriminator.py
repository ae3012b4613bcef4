"""The discriminators of the Vocos training step (``vocoders/vocos/models/discriminator.py``) on native fp32 kernels, with the
reference's constructors, module tree, ``state_dict`` keys and return values: ``DiscriminatorP`` and ``MultiPeriodDiscriminator``
(``:11-75``; an ``mpd_{epoch}.pt`` loads with ``strict=True``), which ``install(discriminator="train")`` rebinds in the user's own
``vocoders.vocos.models.discriminator``, and ``DiscriminatorR`` and ``MultiResolutionDiscriminator`` (``:78-171``; an
``mrd_{epoch}.pt`` loads with ``strict=True``, the ``spec_fn.window`` buffers of torchaudio's ``Spectrogram`` included), which
``install(resolution_discriminator="train")`` rebinds there.  Either keyword leaves the other pair of names alone.

One native handle serves one ``DiscriminatorP`` (st_create_period_discriminator).  The parameters -- the weight norm's ``g`` /
``v`` and the biases -- are bound in place, so an optimizer step costs no copy; the effective weights are recomputed when the
parameters change, not per call.  Under ``torch.no_grad()`` or in ``eval()`` mode a call runs the forward that keeps nothing;
otherwise one ``torch.autograd.Function`` takes the waveform and the 18 parameters to the five feature maps, and its backward
launches only what ``needs_input_grad`` asks for: no weight-gradient kernel for a ``requires_grad_(False)`` module, no input
gradient for ``y_hat.detach()``.  The engine keeps the activations of ONE forward, and each forward can be differentiated once.
Only ``in_channels=1, kernel_size=5, stride=3`` are built natively.  There is no CPU fallback.

``DiscriminatorR`` follows the same rules with one handle per window length (st_create_resolution_discriminator): its function
takes the waveform and the 78 parameters to the 21 feature maps (band-major: layers 1..4 of each of the five bands, then
``conv_post``'s output, which is also the first return value, not flattened).  The complex STFT runs on the native real FFT, so
no torchaudio is needed.  Built natively: ``window_length`` a power of two in [32, 2048], ``channels=32``, ``hop_factor=0.25``,
five ``bands`` whose integer bin ranges are all non-empty, the reference's fixed slope 0.1.
"""
from typing import List, Tuple

import torch
from torch import Tensor, nn
from torch.nn import Conv2d
from torch.nn.utils.parametrizations import weight_norm

from . import _lib
from ._native_module import NativeModule, check_activations_live, param_grad_views

__all__ = ["DiscriminatorP", "MultiPeriodDiscriminator", "DiscriminatorR", "MultiResolutionDiscriminator"]


class _DiscriminatorFn(torch.autograd.Function):
    """A native discriminator's forward under autograd.  Inputs (module, parameter names, x, *parameters) -> its feature maps
    (DiscriminatorP: five, DiscriminatorR: 21)."""

    @staticmethod
    def forward(ctx, mod, names, x, *params):
        eng = mod.engine()
        dev = x.device
        xf = x.detach().to(torch.float32).contiguous()
        fmaps = mod._run(eng, xf, True)
        ctx.mod, ctx.eng, ctx.serial, ctx.vers = mod, eng, eng.train_serial(), mod._param_key()[1]
        ctx.names, ctx.params, ctx.shape, ctx.dev, ctx.x_dtype, ctx.spent = names, params, (xf.shape[0], xf.shape[2]), dev, x.dtype, False
        ctx.set_materialize_grads(False)
        return tuple(fmaps)

    @staticmethod
    def backward(ctx, *grads):
        need = ctx.needs_input_grad
        if all(g is None for g in grads):
            return (None,) * len(need)
        if ctx.spent:
            raise RuntimeError(f"stabletts_amd: this {ctx.mod._noun} forward has been differentiated already -- the native backward runs once "
                               "per forward (its scratch overwrites what a second pass would need); run the forward again")
        mod, eng, dev = ctx.mod, ctx.eng, ctx.dev
        check_activations_live(mod, eng, ctx.serial, ctx.vers)
        ctx.spent = True
        B, T = ctx.shape
        gs = [None if g is None else g.detach().to(device=dev, dtype=torch.float32).contiguous() for g in grads]
        lay = eng.grad_layout()
        with torch.cuda.device(dev):
            flat = torch.zeros(lay[None], device=dev, dtype=torch.float32) if any(need[3:]) else None    # (gaps and unreached slices stay 0)
            d_x = torch.empty(B, 1, T, device=dev, dtype=torch.float32) if need[2] else None
            getattr(eng, mod._native + "_train_backward")(B, T, gs, d_x, flat, torch.cuda.current_stream(dev).cuda_stream)
        if d_x is not None:
            d_x = d_x.to(ctx.x_dtype)
        pg = param_grad_views(flat, lay, ctx.names, ctx.params, need[3:]) if flat is not None else [None] * len(ctx.params)
        return (None, None, d_x) + tuple(pg)


class _Discriminator(NativeModule):
    """What DiscriminatorP and DiscriminatorR share.  A class defines ``_noun`` (its name in messages), ``_native`` (the prefix of
    its ``_lib.Engine`` methods), ``_config()`` (what its handle was created from), ``_fmap_shapes(eng, B, T)`` and, where the
    input has a minimum length, ``_check_input(x)``."""
    native_training = True

    def engine(self):
        eng = self._engine
        if eng is not None and getattr(eng, "disc_config", None) != self._config():
            eng.close()                      # the configuration was re-assigned after construction: another handle
            self._engine = None
        eng = super().engine()
        eng.disc_config = self._config()
        return eng

    def _check_input(self, x):
        pass

    def _run(self, eng, xf, train):
        B, _, T = xf.shape
        dev = xf.device
        with torch.cuda.device(dev):
            fmaps = [torch.empty(s, device=dev, dtype=torch.float32) for s in self._fmap_shapes(eng, B, T)]
            getattr(eng, self._native + "_forward")(xf, fmaps, train, torch.cuda.current_stream(dev).cuda_stream)
        return fmaps

    def _feature_maps(self, x: Tensor) -> List[Tensor]:
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            self.engine()      # raises: no CPU fallback
        if x.device != dev:
            raise ValueError(f"the input is on {x.device}, the {self._what}'s parameters are on {dev}")
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError("x must be (B, 1, T)")
        self._check_input(x)
        if self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            named = list(self.named_parameters())
            return list(_DiscriminatorFn.apply(self, [n for n, _ in named], x, *[p for _, p in named]))
        with torch.no_grad():
            return self._run(self.engine(), x.detach().to(torch.float32).contiguous(), False)


class _MultiDiscriminator(nn.Module):
    """``forward`` of MultiPeriodDiscriminator and MultiResolutionDiscriminator over ``self.discriminators``."""

    def forward(self, y: Tensor, y_hat: Tensor) -> Tuple[List[Tensor], List[Tensor], List[List[Tensor]], List[List[Tensor]]]:
        """As the reference: (y_d_rs, y_d_gs, fmap_rs, fmap_gs).  Every discriminator runs ONCE on cat([y, y_hat]) -- the weights are
        read once and each engine holds one forward -- and the halves come back as views, bitwise what each signal gives alone."""
        if y.shape[1:] != y_hat.shape[1:]:
            raise ValueError(f"y {tuple(y.shape)} and y_hat {tuple(y_hat.shape)} must agree in every dimension but the batch")
        n = y.shape[0]
        x = torch.cat([y, y_hat.to(y.dtype)], dim=0)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for d in self.discriminators:
            logits, fmap = d(x)
            y_d_rs.append(logits[:n])
            y_d_gs.append(logits[n:])
            fmap_rs.append([f[:n] for f in fmap])
            fmap_gs.append([f[n:] for f in fmap])
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs


class DiscriminatorP(_Discriminator):
    _what = "period discriminator"
    _noun = "DiscriminatorP"
    _native = "period_disc"

    def __init__(self, period: int, in_channels: int = 1, kernel_size: int = 5, stride: int = 3, lrelu_slope: float = 0.1):
        super().__init__()
        if (in_channels, kernel_size, stride) != (1, 5, 3):
            raise NotImplementedError("the native DiscriminatorP is built for in_channels=1, kernel_size=5, stride=3 "
                                      f"(got in_channels={in_channels}, kernel_size={kernel_size}, stride={stride})")
        if not lrelu_slope > 0:
            raise NotImplementedError("the native DiscriminatorP needs lrelu_slope > 0 (its backward reads the pre-activation's sign "
                                      "from the post-activation)")
        self.period = period
        pad = (kernel_size // 2, 0)
        self.convs = nn.ModuleList([
            weight_norm(Conv2d(in_channels, 32, (kernel_size, 1), (stride, 1), padding=pad)),
            weight_norm(Conv2d(32, 128, (kernel_size, 1), (stride, 1), padding=pad)),
            weight_norm(Conv2d(128, 512, (kernel_size, 1), (stride, 1), padding=pad)),
            weight_norm(Conv2d(512, 1024, (kernel_size, 1), (stride, 1), padding=pad)),
            weight_norm(Conv2d(1024, 1024, (kernel_size, 1), (1, 1), padding=pad)),
        ])
        self.conv_post = weight_norm(Conv2d(1024, 1, (3, 1), 1, padding=(1, 0)))
        self.lrelu_slope = lrelu_slope

    def _create_engine(self, dev):
        return _lib.Engine(0, 0, 0, 0, 0, 0, 0, self.operand_dtype, dev,
                           period_discriminator=dict(period=self.period, lrelu_slope=self.lrelu_slope))

    def _config(self):
        return (self.period, float(self.lrelu_slope))

    def _fmap_shapes(self, eng, B, T):
        return eng.period_disc_fmap_shapes(B, T, self.period)

    def forward(self, x: Tensor) -> Tuple[Tensor, List[Tensor]]:
        """x (B, 1, T) -> (logits (B, H * period), [the four feature maps after convs.1..4, conv_post's output])."""
        fmap = self._feature_maps(x)
        return torch.flatten(fmap[-1], 1, -1), fmap


class MultiPeriodDiscriminator(_MultiDiscriminator):
    def __init__(self, periods: Tuple[int, ...] = (2, 3, 5, 7, 11)):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorP(period=p) for p in periods])


class _SpectrogramWindow(nn.Module):
    """What the reference's ``spec_fn`` (torchaudio's ``Spectrogram``) contributes to a ``state_dict``: its persistent ``window``
    buffer, ``hann_window(window_length)``.  An ``mrd_{epoch}.pt`` carries ``discriminators.{k}.spec_fn.window``, and a checkpoint
    saved here loads into the reference.  The transform itself runs in the engine, which computes the same window."""

    def __init__(self, window_length: int):
        super().__init__()
        self.register_buffer("window", torch.hann_window(window_length))


class DiscriminatorR(_Discriminator):
    _what = "resolution discriminator"
    _noun = "DiscriminatorR"
    _native = "resolution_disc"
    lrelu_slope = 0.1           # the reference hard-codes it (discriminator.py:163); an instance may override it before its first call

    def __init__(self, window_length: int, channels: int = 32, hop_factor: float = 0.25,
                 bands: Tuple[Tuple[float, float], ...] = ((0.0, 0.1), (0.1, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0))):
        super().__init__()
        limits = ("the native DiscriminatorR is built for window_length a power of two in [32, 2048], channels=32, hop_factor=0.25 and "
                  "five bands whose integer bin ranges int(b * (window_length // 2 + 1)) are all non-empty and inside the spectrum")
        if (not isinstance(window_length, int) or window_length < 32 or window_length > 2048 or window_length & (window_length - 1)
                or channels != 32 or hop_factor != 0.25 or len(bands) != 5):
            raise NotImplementedError(f"{limits} (got window_length={window_length}, channels={channels}, hop_factor={hop_factor}, "
                                      f"{len(bands)} bands)")
        self.window_length = window_length
        self.hop_factor = hop_factor
        self.spec_fn = _SpectrogramWindow(window_length)
        n_fft = window_length // 2 + 1
        bands = [(int(b[0] * n_fft), int(b[1] * n_fft)) for b in bands]
        if any(lo < 0 or hi > n_fft or hi <= lo for lo, hi in bands):
            raise NotImplementedError(f"{limits} (got the bin ranges {bands} of {n_fft} bins)")
        self.bands = bands
        convs = lambda: nn.ModuleList([                                            # noqa: E731
            weight_norm(nn.Conv2d(2, channels, (3, 9), (1, 1), padding=(1, 4))),
            weight_norm(nn.Conv2d(channels, channels, (3, 9), (1, 2), padding=(1, 4))),
            weight_norm(nn.Conv2d(channels, channels, (3, 9), (1, 2), padding=(1, 4))),
            weight_norm(nn.Conv2d(channels, channels, (3, 9), (1, 2), padding=(1, 4))),
            weight_norm(nn.Conv2d(channels, channels, (3, 3), (1, 1), padding=(1, 1))),
        ])
        self.band_convs = nn.ModuleList([convs() for _ in range(len(self.bands))])
        self.conv_post = weight_norm(nn.Conv2d(channels, 1, (3, 3), (1, 1), padding=(1, 1)))

    def _config(self):
        return (self.window_length, tuple(tuple(b) for b in self.bands), float(self.lrelu_slope))

    def _create_engine(self, dev):
        cfg = dict(window_length=self.window_length, lrelu_slope=self.lrelu_slope)
        for c, (lo, hi) in enumerate(self.bands):
            cfg[f"band_lo{c}"], cfg[f"band_hi{c}"] = lo, hi
        return _lib.Engine(0, 0, 0, 0, 0, 0, 0, self.operand_dtype, dev, resolution_discriminator=cfg)

    def _fmap_shapes(self, eng, B, T):
        return eng.resolution_disc_fmap_shapes(B, T)

    def _check_input(self, x):
        if x.shape[2] <= self.window_length // 2:
            raise ValueError(f"T = {x.shape[2]} is too short for window_length {self.window_length}: the reflect padding of "
                             f"{self.window_length // 2} samples needs T > {self.window_length // 2}")

    def forward(self, x: Tensor) -> Tuple[Tensor, List[Tensor]]:
        """x (B, 1, T) -> (logits (B, 1, frames, F'), [layers 1..4 of band 0, .. of band 4, conv_post's output]): 21 maps, the last
        being the first return value itself."""
        fmap = self._feature_maps(x)
        return fmap[-1], fmap


class MultiResolutionDiscriminator(_MultiDiscriminator):
    def __init__(self, fft_sizes: Tuple[int, ...] = (2048, 1024, 512)):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorR(window_length=w) for w in fft_sizes])
