"""Drop-in replacement for the reference's ``models/duration_predictor.py``: ``DurationPredictor`` (stage 3 of
``StableTTS.synthesise``, models/model.py:81) and ``duration_loss`` (the two names models/model.py:9 imports).

Same constructor (duration_predictor.py:6) and checkpoint keys (``conv1``, ``norm1``, ``conv2``, ``norm2``, ``proj``,
``cond``), ``forward(x, x_mask, g)`` as :24.  The forward pass runs in fp32 on gfx950 kernels behind
``st_duration_predictor_forward`` (include/stabletts_hip.h): logw feeds ``ceil(exp(logw))``, where a 16-bit error would add
or drop whole frames.  Eval-mode semantics (no dropout); there is no PyTorch fallback.  Grad-enabled calls raise unless ``native_training`` is
set (``install(duration_predictor="train")`` registers ``duration_predictor_train``, whose DurationPredictor sets it): then
they run the native training forward / backward with the reference's train-mode dropout.
"""
import torch
import torch.nn as nn

from ._fp32_module import NativeFp32Module, _DurationPredictorFn


class DurationPredictor(NativeFp32Module):
    _what = "DurationPredictor"
    _engine_kwarg = "duration_predictor"

    def __init__(self, in_channels, filter_channels, kernel_size, p_dropout, gin_channels=0):
        super().__init__()
        self.in_channels = in_channels
        self.filter_channels = filter_channels
        self.kernel_size = kernel_size
        self.p_dropout = p_dropout
        self.gin_channels = gin_channels
        self.drop = nn.Dropout(p_dropout)
        self.conv1 = nn.Conv1d(in_channels, filter_channels, kernel_size, padding=kernel_size // 2)
        self.norm1 = nn.LayerNorm(filter_channels)
        self.conv2 = nn.Conv1d(filter_channels, filter_channels, kernel_size, padding=kernel_size // 2)
        self.norm2 = nn.LayerNorm(filter_channels)
        self.proj = nn.Conv1d(filter_channels, 1, 1)
        self.cond = nn.Conv1d(gin_channels, in_channels, 1)

    def _native_config(self):
        return dict(in_channels=self.in_channels, filter_channels=self.filter_channels, kernel_size=self.kernel_size,
                    gin_channels=self.gin_channels)

    def forward(self, x, x_mask, g):
        """x: (B, in_channels, Tx), x_mask: (B, 1, Tx), g: (B, gin_channels) -> logw (B, 1, Tx), 0 at padded tokens."""
        # x and g are detached in the reference (:25-26): only the parameters could ask for a backward
        dev = self._check_call((x_mask,))
        for t in (x, g):
            if t.device != dev:
                raise ValueError(f"an input is on {t.device}, the DurationPredictor's parameters are on {dev}")
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError("x must be (B, in_channels, Tx)")
        B, _, T = x.shape
        if x_mask.numel() != B * T or g.shape != (B, self.gin_channels):
            raise ValueError("x_mask must be (B, 1, Tx) and g (B, gin_channels)")
        if self._training_call((x_mask,)):
            xx = x.detach().to(torch.float32).contiguous()
            mm = x_mask.detach().to(torch.float32).reshape(B, 1, T).contiguous()
            gg = g.detach().to(torch.float32).contiguous()
            names, params = zip(*self.named_parameters())
            return _DurationPredictorFn.apply(self, names, xx, mm, gg, *params)
        with torch.no_grad():
            eng = self.engine()
            xx = x.detach().to(torch.float32).contiguous()
            mm = x_mask.detach().to(torch.float32).reshape(B, 1, T).contiguous()
            gg = g.detach().to(torch.float32).contiguous()
            logw = torch.empty(B, 1, T, device=dev, dtype=torch.float32)
            with torch.cuda.device(dev):
                eng.duration_predictor_forward(xx, mm, gg, logw, torch.cuda.current_stream(dev).cuda_stream)
            return logw


def duration_loss(logw, logw_, lengths):
    """Sum of squared log-duration errors over the total number of tokens (the reference's duration_loss)."""
    return ((logw - logw_) ** 2).sum() / lengths.sum()
