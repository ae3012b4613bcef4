"""Drop-in replacement for the reference's ``models/text_encoder.py`` (the caller side
of the hot path, on the same DiT block kernels).

``TextEncoder`` keeps the reference constructor (models/text_encoder.py:9), the ``forward(x, c, x_lengths)``
signature (:34) and the checkpoint key layout (``emb.weight``, ``encoder.<i>.attn.conv_q.weight``, ...,
``proj.bias``), but embedding, the ``n_layers`` DiTConVBlocks (adaLN-Zero, RoPE attention, conv-FFN) and the
output projection run as hand-written gfx950 kernels behind ``st_text_encoder_forward``
(include/stabletts_hip.h); there is no PyTorch fallback.

Under autograd (a parameter or ``c`` requires grad) the forward is ``st_text_encoder_train_forward``, which keeps the
activations in the engine, and ``loss.backward()`` runs ``st_text_encoder_train_backward``: every parameter gradient
(``emb.weight`` included) is a view of one flat buffer the kernels wrote, and ``c`` receives d loss / d c.  Train-mode
dropout is counter-based with a seed drawn from torch's CPU generator, as in the decoder's training path.
"""
import torch
import torch.nn as nn

from . import _lib
from ._native_module import NativeModule, check_activations_live, dropout_seed, param_grad_views
from .estimator import DiTConVBlock


class TextEncoder(NativeModule):
    """engine(): as the decoder's (estimator.py): the engine reads the fp32 parameters in place (st_bind_param) and, after an
    in-place update such as an optimizer step, re-packs its 16-bit copies on the current stream (st_repack): no re-upload, no
    allocation."""
    _what = "text encoder"

    def __init__(self, n_vocab, out_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size,
                 p_dropout, gin_channels, operand_dtype="f16"):
        super().__init__()
        self.n_vocab, self.out_channels, self.hidden_channels = n_vocab, out_channels, hidden_channels
        self.filter_channels, self.n_heads, self.n_layers = filter_channels, n_heads, n_layers
        self.kernel_size, self.p_dropout, self.gin_channels = kernel_size, p_dropout, gin_channels
        self.operand_dtype = operand_dtype
        self.scale = self.hidden_channels ** 0.5

        self.emb = nn.Embedding(n_vocab, hidden_channels)
        nn.init.normal_(self.emb.weight, 0.0, hidden_channels ** -0.5)
        self.encoder = nn.ModuleList([DiTConVBlock(hidden_channels, filter_channels, n_heads, kernel_size, gin_channels)
                                      for _ in range(n_layers)])
        self.proj = nn.Conv1d(hidden_channels, out_channels, 1)
        self.initialize_weights()

    def initialize_weights(self):
        """adaLN-Zero (models/text_encoder.py:29-32)."""
        for block in self.encoder:
            nn.init.constant_(block.adaLN_modulation[-1].weight, 0)
            nn.init.constant_(block.adaLN_modulation[-1].bias, 0)

    def _create_engine(self, dev):
        return _lib.Engine(self.out_channels, self.hidden_channels, self.filter_channels, self.n_heads, self.n_layers,
                           self.kernel_size, self.gin_channels, self.operand_dtype, dev, text_encoder_vocab=self.n_vocab)

    def forward(self, x: torch.Tensor, c: torch.Tensor, x_lengths: torch.Tensor):
        """x: (B, T) phoneme ids, c: (B, gin) speaker vectors, x_lengths: (B,) ->
        (x (B, hidden, T), mu_x (B, out, T), x_mask (B, 1, T)) exactly as models/text_encoder.py:34-44."""
        if self.emb.weight.device.type != "cuda":
            self.engine()      # raises: no CPU fallback
        if torch.is_grad_enabled() and (c.requires_grad or any(p.requires_grad for p in self.parameters())):
            names, params = zip(*self.named_parameters())
            return _TextEncoderFn.apply(self, names, x, c, x_lengths, *params)
        with torch.no_grad():
            return self._forward(x, c, x_lengths)

    def _inputs(self, x, c, x_lengths):
        dev = self.emb.weight.device
        for name, t in (("x", x), ("c", c), ("x_lengths", x_lengths)):
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the encoder's parameters are on {dev}")
        if x.dim() != 2 or c.shape != (x.shape[0], self.gin_channels) or x_lengths.shape != (x.shape[0],):
            raise ValueError("shape mismatch: x (B,T) ids, c (B,gin), x_lengths (B,)")
        B, T = x.shape
        tok = x.detach().to(device=dev, dtype=torch.long).contiguous()
        lens = x_lengths.detach().to(device=dev, dtype=torch.long).contiguous()
        cc = c.detach().to(device=dev, dtype=torch.float32).contiguous()
        return dev, tok, lens, cc

    def _forward(self, x, c, x_lengths):
        eng = self.engine()
        dev, tok, lens, cc = self._inputs(x, c, x_lengths)
        B, T = tok.shape
        h = torch.empty(B, self.hidden_channels, T, device=dev, dtype=torch.float32)
        mu_x = torch.empty(B, self.out_channels, T, device=dev, dtype=torch.float32)
        mask = torch.empty(B, 1, T, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            eng.text_encoder_forward(tok, lens, cc, h, mu_x, mask, torch.cuda.current_stream(dev).cuda_stream)
        return h, mu_x, mask


class _TextEncoderFn(torch.autograd.Function):
    """TextEncoder.forward under autograd: st_text_encoder_train_forward keeps the activations in the engine, the backward is
    st_text_encoder_train_backward.  Inputs (module, names, ids, c, lengths, *parameters); outputs (x, mu_x, x_mask)."""

    @staticmethod
    def forward(ctx, mod, names, x, c, x_lengths, *params):
        eng = mod.engine()
        dev, tok, lens, cc = mod._inputs(x, c, x_lengths)
        B, T = tok.shape
        f32 = dict(device=dev, dtype=torch.float32)
        h = torch.empty(B, mod.hidden_channels, T, **f32)
        mu_x = torch.empty(B, mod.out_channels, T, **f32)
        mask = torch.empty(B, 1, T, **f32)
        p_drop = float(mod.p_dropout) if mod.training else 0.0
        seed = dropout_seed(p_drop)
        with torch.cuda.device(dev):
            eng.text_encoder_train_forward(tok, lens, cc, h, mu_x, mask, p_drop, seed, torch.cuda.current_stream(dev).cuda_stream)
        ctx.mod, ctx.eng, ctx.serial, ctx.vers = mod, eng, eng.train_serial(), mod._param_key()[1]
        ctx.names, ctx.params, ctx.shape, ctx.dev, ctx.c_shape = names, params, (B, T), dev, tuple(cc.shape)
        ctx.mark_non_differentiable(mask)
        ctx.set_materialize_grads(False)
        return h, mu_x, mask

    @staticmethod
    def backward(ctx, grad_x, grad_mu, _grad_mask):
        mod, eng = ctx.mod, ctx.eng
        check_activations_live(mod, eng, ctx.serial, ctx.vers)
        need = ctx.needs_input_grad          # (mod, names, x, c, x_lengths, *params)
        if grad_x is None and grad_mu is None:
            return (None,) * len(need)
        dev = ctx.dev
        B, T = ctx.shape
        prep = lambda g: g.detach().to(device=dev, dtype=torch.float32).contiguous() if g is not None else None      # noqa: E731
        gx, gmu = prep(grad_x), prep(grad_mu)
        lay = eng.grad_layout()
        with torch.cuda.device(dev):
            # (zeros, not empty: the 64-byte alignment gaps between the slices are never written)
            flat = torch.zeros(lay[None], device=dev, dtype=torch.float32)
            gc = torch.empty(ctx.c_shape, device=dev, dtype=torch.float32) if need[3] else None
            eng.text_encoder_train_backward(ctx.serial, B, T, gx, gmu, flat, gc, torch.cuda.current_stream(dev).cuda_stream)
        return (None, None, None, gc, None, *param_grad_views(flat, lay, ctx.names, ctx.params, need[5:]))
