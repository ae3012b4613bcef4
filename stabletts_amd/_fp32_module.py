"""Shared plumbing of the native fp32 modules (MelStyleEncoder, DurationPredictor): a parameter container whose forward runs
in libstabletts_hip.so.  The handle is created on the parameters' device and re-reads the weights whenever their storage or
version counters change, as text_encoder.TextEncoder does.  There is no CPU fallback.

Training is opt-in per instance: with ``native_training`` set (the subclasses that ``install(reference_encoder="train")`` /
``install(duration_predictor="train")`` register), a grad-enabled call runs the native training forward and backward
(``_StyleEncoderFn`` / ``_DurationPredictorFn``) and the engine reads the parameters in place (st_bind_param), so an optimizer
step costs no copy and no host synchronisation.  Without it a grad-enabled call raises NotImplementedError, as before."""
import torch

from . import _lib
from ._native_module import NativeModule, check_activations_live, dropout_seed, param_grad_views


class NativeFp32Module(NativeModule):
    _rebind = False             # st_load_param copies: every change re-loads (native_training: bound in place, see _sync)
    _engine_kwarg = None        # _lib.Engine keyword selecting the handle kind
    native_training = False     # opt-in: grad-enabled calls train on the native kernels (instance / subclass attribute)

    def _native_config(self):  # pragma: no cover
        raise NotImplementedError

    def _create_engine(self, dev):
        return _lib.Engine(0, 0, 0, 0, 0, 0, 0, self.operand_dtype, dev, **{self._engine_kwarg: self._native_config()})

    def _sync(self, dev):
        if self.native_training:
            # bound in place: a new storage (first use, .to(), re-assignment) re-binds; an in-place update needs nothing
            named = list(self.named_parameters())
            if all(p.dtype == torch.float32 and p.is_contiguous() for _, p in named):
                key = self._param_key()
                if key[0] != (self._engine_key[0] if self._engine_key else None):
                    with torch.no_grad():
                        self._engine.bind_parameters([(n, p.detach()) for n, p in named])    # st_finalize synchronises once
                self._engine_key = key
                return
        super()._sync(dev)

    def _training_call(self, tensors):
        """True when this call must run the native training path (grad-enabled, something requires grad, opted in)."""
        return (self.native_training and torch.is_grad_enabled()
                and (any(t.requires_grad for t in tensors if t is not None) or any(p.requires_grad for p in self.parameters())))

    def _check_call(self, tensors):
        """Raises before any work: grad-enabled calls that would need a backward (unless native_training), tensors off the
        parameters' device."""
        if not self.native_training and torch.is_grad_enabled() and (any(t.requires_grad for t in tensors if t is not None)
                                                                     or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(f"the native {self._what} is inference-only (no backward kernels): call it under "
                                      "torch.no_grad(), train with the reference module and load its checkpoint, or opt in to "
                                      "native training (native_training = True; stabletts_amd.install(reference_encoder=\"train\", "
                                      "duration_predictor=\"train\"))")
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            self.engine()      # raises: no CPU fallback
        for t in tensors:
            if t is not None and t.device != dev:
                raise ValueError(f"an input is on {t.device}, the {self._what}'s parameters are on {dev}")
        return dev


class _TrainFn(torch.autograd.Function):
    """A native fp32 module's forward under autograd: the engine's ``<kind>_train_forward`` keeps the activations, the backward
    is its ``<kind>_train_backward``.  Inputs (module, names, the n_in input tensors, *parameters), ``out_shape(mod, B, T)``
    the one output's.  The inputs are data (the reference detaches them, or they are the mel): no input gradient."""
    kind, n_in, p_attr = None, 0, "p_dropout"

    @classmethod
    def forward(cls, ctx, mod, names, *args):
        inputs, params = args[:cls.n_in], args[cls.n_in:]
        eng = mod.engine()
        dev = inputs[0].device
        B, _, T = inputs[0].shape
        out = torch.empty(cls.out_shape(mod, B, T), device=dev, dtype=torch.float32)
        p_drop = float(getattr(mod, cls.p_attr)) if mod.training else 0.0
        with torch.cuda.device(dev):
            getattr(eng, cls.kind + "_train_forward")(*inputs, out, p_drop, dropout_seed(p_drop), torch.cuda.current_stream(dev).cuda_stream)
        ctx.mod, ctx.eng, ctx.serial, ctx.vers = mod, eng, eng.train_serial(), mod._param_key()[1]
        ctx.names, ctx.params, ctx.shape, ctx.dev = names, params, (B, T), dev
        ctx.set_materialize_grads(False)
        return out

    @classmethod
    def backward(cls, ctx, grad):
        check_activations_live(ctx.mod, ctx.eng, ctx.serial, ctx.vers)
        need = ctx.needs_input_grad
        if grad is None:
            return (None,) * len(need)
        eng, dev = ctx.eng, ctx.dev
        g = grad.detach().to(device=dev, dtype=torch.float32).contiguous()
        lay = eng.grad_layout()
        with torch.cuda.device(dev):
            flat = torch.zeros(lay[None], device=dev, dtype=torch.float32)     # (the alignment gaps stay 0)
            getattr(eng, cls.kind + "_train_backward")(ctx.serial, *ctx.shape, g, flat, torch.cuda.current_stream(dev).cuda_stream)
        return (None,) * (2 + cls.n_in) + tuple(param_grad_views(flat, lay, ctx.names, ctx.params, need[2 + cls.n_in:]))


class _StyleEncoderFn(_TrainFn):
    """MelStyleEncoder: (mel, mask) -> c."""
    kind, n_in, p_attr = "style_encoder", 2, "dropout"
    out_shape = staticmethod(lambda mod, B, T: (B, mod.out_dim))


class _DurationPredictorFn(_TrainFn):
    """DurationPredictor: (x, x_mask, g) -> logw."""
    kind, n_in = "duration_predictor", 3
    out_shape = staticmethod(lambda mod, B, T: (B, 1, T))
