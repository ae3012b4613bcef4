"""Drop-in replacement for the reference's ``models/reference_encoder.py``: ``MelStyleEncoder`` (stage 1 of
``StableTTS.synthesise``, models/model.py:79) and its ``Conv1dGLU``.

Same constructor (reference_encoder.py:25-33) and checkpoint keys (``spectral.0.weight``, ``temporal.<i>.conv1.weight``,
``slf_attn.in_proj_weight``, ``slf_attn.out_proj.weight``, ``fc.weight``, ...), ``forward(x, x_mask=None)`` as :74.  The
forward pass runs in fp32 on gfx950 kernels behind ``st_style_encoder_forward`` (include/stabletts_hip.h); eval-mode
semantics (no dropout).  There is no PyTorch fallback.  Grad-enabled calls raise unless ``native_training`` is set
(``install(reference_encoder="train")`` registers ``reference_encoder_train``, whose MelStyleEncoder sets it): then they run
the native training forward / backward, with the reference's train-mode dropout.  An item whose ``x_mask`` has no valid frame gives
NaN, like the reference's 0 / 0.
"""
import torch
import torch.nn as nn

from ._fp32_module import NativeFp32Module, _StyleEncoderFn
from .estimator import _ParamsOnly


class Conv1dGLU(_ParamsOnly):
    """reference_encoder.py:4-20 (parameters only): k-tap conv to 2 x out_channels, value * sigmoid(gate) + residual."""
    def __init__(self, in_channels, out_channels, kernel_size, dropout):
        super().__init__()
        self.out_channels = out_channels
        self.conv1 = nn.Conv1d(in_channels, 2 * out_channels, kernel_size=kernel_size, padding=kernel_size // 2)
        self.dropout = nn.Dropout(dropout)


class MelStyleEncoder(NativeFp32Module):
    _what = "MelStyleEncoder"
    _engine_kwarg = "style_encoder"

    def __init__(self, n_mel_channels=80, style_hidden=128, style_vector_dim=256, style_kernel_size=5, style_head=2, dropout=0.1):
        super().__init__()
        self.in_dim = n_mel_channels
        self.hidden_dim = style_hidden
        self.out_dim = style_vector_dim
        self.kernel_size = style_kernel_size
        self.n_head = style_head
        self.dropout = dropout
        self.spectral = nn.Sequential(
            nn.Linear(self.in_dim, self.hidden_dim), nn.Mish(inplace=True), nn.Dropout(self.dropout),
            nn.Linear(self.hidden_dim, self.hidden_dim), nn.Mish(inplace=True), nn.Dropout(self.dropout),
        )
        self.temporal = nn.Sequential(
            Conv1dGLU(self.hidden_dim, self.hidden_dim, self.kernel_size, self.dropout),
            Conv1dGLU(self.hidden_dim, self.hidden_dim, self.kernel_size, self.dropout),
        )
        self.slf_attn = nn.MultiheadAttention(self.hidden_dim, self.n_head, self.dropout, batch_first=True)
        self.fc = nn.Linear(self.hidden_dim, self.out_dim)

    def _native_config(self):
        return dict(n_mel_channels=self.in_dim, style_hidden=self.hidden_dim, style_vector_dim=self.out_dim,
                    style_kernel_size=self.kernel_size, style_head=self.n_head)

    def forward(self, x, x_mask=None):
        """x: (B, n_mel_channels, T) mel, x_mask: (B, 1, T) or None -> (B, style_vector_dim)  (reference_encoder.py:74-93)."""
        dev = self._check_call((x, x_mask))
        if x.dim() != 3 or x.shape[1] != self.in_dim:
            raise ValueError("x must be (B, n_mel_channels, T)")
        B, _, T = x.shape
        if x_mask is not None and x_mask.numel() != B * T:
            raise ValueError("x_mask must be (B, 1, T)")
        if self._training_call((x, x_mask)):
            mel = x.detach().to(torch.float32).contiguous()
            mask = x_mask.detach().to(torch.float32).reshape(B, 1, T).contiguous() if x_mask is not None else None
            names, params = zip(*self.named_parameters())
            return _StyleEncoderFn.apply(self, names, mel, mask, *params)
        with torch.no_grad():
            eng = self.engine()
            mel = x.detach().to(torch.float32).contiguous()
            mask = x_mask.detach().to(torch.float32).reshape(B, 1, T).contiguous() if x_mask is not None else None
            c = torch.empty(B, self.out_dim, device=dev, dtype=torch.float32)
            with torch.cuda.device(dev):
                eng.style_encoder_forward(mel, mask, c, torch.cuda.current_stream(dev).cuda_stream)
            return c
