"""``vocoders.vocos.models.model`` for Vocos training (``install(vocoder="train")``): the same module as ``vocos`` -- constructor,
module tree, state_dict keys, inference path -- but ``Vocos.native_training = True``: its parameters require grad, and a
grad-enabled call in train mode runs the native fp32 training forward (st_vocos_train_forward, which keeps its activations) with
st_vocos_train_backward as its backward: d audio -> the gradient of every parameter and of the mel, with no torch kernel between
the mel and the gradients.  This is the generator of vocoders/vocos/train.py:94,115,128, at the trainer's own configuration
(vocoders/vocos/config.py:21-26: dim 768, intermediate_dim 2048, 12 layers) as at the inference preset (dim 512, 768 or 1024); the discriminators (torch, or the native multi-period one of
``stabletts_amd.discriminator``) consume the returned waveform as an ordinary autograd tensor.

The training path is fp32 throughout (fp32-input MFMA GEMMs), so its waveform is NOT bitwise the inference waveform, whose GEMMs
run on f16 / bf16 operands: it is closer to the reference's than the inference one.  The engine reads the parameters in place
(st_bind_param), so an optimizer step costs no copy; the 16-bit copies of the inference path are packed again only when a
no_grad / eval call follows a parameter update.  Under ``torch.no_grad()`` or in ``eval()`` mode a call is the inference path of
``stabletts_amd.vocos``, unchanged.  Training is built for n_fft 2048 / hop_length 512 and input_channels 64, 128 or 192: at the
other configurations the inference path takes (n_fft 256-1024, mel widths in steps of 16) the module still constructs, loads and
vocodes under ``no_grad``, and a grad-enabled call raises the ``NativeError`` of ``ST_ERR_UNSUPPORTED``.  The engine keeps the activations of ONE training forward, and each forward can be
differentiated once.
"""
import torch

from ._native_module import check_activations_live, param_grad_views
from .vocos import ISTFT, ISTFTHead, ConvNeXtBlock, VocosBackbone  # noqa: F401  (the names of vocos)
from .vocos import Vocos as _Vocos

_WINDOW = "head.istft.window"


class _VocosFn(torch.autograd.Function):
    """Vocos.forward under autograd.  Inputs (module, parameter names, mel, *parameters) -> audio (B, T * hop_length)."""

    @staticmethod
    def forward(ctx, mod, names, mel, *params):
        eng = mod.engine()
        dev = mel.device
        x = mel.detach().to(torch.float32).contiguous()
        B, _, T = x.shape
        audio = torch.empty(B, T * mod.cfg["hop_length"], device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            eng.vocos_train_forward(x, audio, torch.cuda.current_stream(dev).cuda_stream)
        ctx.mod, ctx.eng, ctx.serial, ctx.vers = mod, eng, eng.train_serial(), mod._param_key()[0][1]
        ctx.names, ctx.params, ctx.shape, ctx.dev, ctx.mel_dtype, ctx.spent = names, params, (B, T), dev, mel.dtype, False
        ctx.set_materialize_grads(False)
        return audio

    @staticmethod
    def backward(ctx, grad):
        need = ctx.needs_input_grad
        if grad is None:
            return (None,) * len(need)
        if ctx.spent:
            raise RuntimeError("stabletts_amd: this Vocos forward has been differentiated already -- the native backward runs once per "
                               "forward (its scratch overwrites what a second pass would need); run the forward again")
        mod = ctx.mod
        updated = mod._param_key()[0][1] != ctx.vers         # a parameter update since the forward: no serial matches (they start at 1)
        check_activations_live(mod, ctx.eng, -1 if updated else ctx.serial)
        ctx.spent = True
        eng, dev = ctx.eng, ctx.dev
        B, T = ctx.shape
        g = grad.detach().to(device=dev, dtype=torch.float32).contiguous()
        lay = eng.grad_layout()
        with torch.cuda.device(dev):
            flat = torch.zeros(lay[None], device=dev, dtype=torch.float32)     # (the alignment gaps and the window's slice stay 0)
            d_mel = torch.empty(B, mod.cfg["input_channels"], T, device=dev, dtype=torch.float32) if need[2] else None
            eng.vocos_train_backward(B, T, g, d_mel, flat, torch.cuda.current_stream(dev).cuda_stream)
        if d_mel is not None:
            d_mel = d_mel.to(ctx.mel_dtype)
        return (None, None, d_mel) + tuple(param_grad_views(flat, lay, ctx.names, ctx.params, need[3:]))


class Vocos(_Vocos):
    native_training = True

    def __init__(self, vocos_config, mel_config, operand_dtype="f16"):
        super().__init__(vocos_config, mel_config, operand_dtype)
        self.requires_grad_(True)
        self._want_packed = True

    def _sync(self, dev):
        """Binds the fp32 parameters and the window in place.  A new storage (first use, .to(), re-assignment) re-binds, which
        also packs the inference path's 16-bit copies; an in-place update (optimizer step) needs nothing for a training call and
        one re-pack (st_finalize) before the next inference call."""
        named = list(self.named_parameters()) + [(_WINDOW, self.head.istft.window)]
        if not all(t.dtype == torch.float32 and t.is_contiguous() for _, t in named):
            return super()._sync(dev)                   # e.g. a .half() module: fp32 copies, re-loaded after every change
        key = self._param_key()
        ptrs = (key[0][0], key[1])
        if not isinstance(self._engine_key, tuple) or len(self._engine_key) != 2 or self._engine_key[0] != ptrs:
            with torch.no_grad():
                torch.cuda.synchronize(dev)
                self._engine.bind_parameters([(n, t.detach()) for n, t in named])
            self._engine_key = (ptrs, key)
        elif self._want_packed and self._engine_key[1] != key:
            self._engine.finalize()
            self._engine_key = (ptrs, key)

    def forward(self, x):
        """mel (B, input_channels, T) -> audio (B, T * hop_length); differentiable in the parameters and the mel in train mode."""
        if not (self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            self._want_packed = True
            with torch.no_grad():
                return super().forward(x)
        dev = next(self.parameters()).device
        if x.device != dev:
            raise ValueError(f"mel is on {x.device}, the vocoder's parameters are on {dev}")
        if x.dim() != 3 or x.shape[1] != self.cfg["input_channels"]:
            raise ValueError("mel must be (B, input_channels, T)")
        named = list(self.named_parameters())
        self._want_packed = False
        try:
            return _VocosFn.apply(self, [n for n, _ in named], x, *[p for _, p in named])
        finally:
            self._want_packed = True

    def forward_ragged(self, x, lengths):
        """``vocos.Vocos.forward_ragged`` on the inference kernels (under ``no_grad``).  The native training forward has no
        ragged form: a call that would have to be differentiated (train mode, grad enabled, something requires grad) raises."""
        if self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("the native training forward has no ragged form (st_vocos_train_forward vocodes at the padded "
                                      "length): call forward_ragged in eval mode or under torch.no_grad()")
        self._want_packed = True
        with torch.no_grad():
            return super().forward_ragged(x, lengths)
