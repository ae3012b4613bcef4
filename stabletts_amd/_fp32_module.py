"""Shared plumbing of the native fp32 modules (MelStyleEncoder, DurationPredictor): a parameter container whose forward runs
in libstabletts_hip.so.  The handle is created on the parameters' device and re-reads the weights whenever their storage or
version counters change, as text_encoder.TextEncoder does.  There is no CPU fallback.

Training is opt-in per instance: with ``native_training`` set (the subclasses that ``install(reference_encoder="train")`` /
``install(duration_predictor="train")`` register), a grad-enabled call runs the native training forward and backward
(``_StyleEncoderFn`` / ``_DurationPredictorFn``) and the engine reads the parameters in place (st_bind_param), so an optimizer
step costs no copy and no host synchronisation.  Without it a grad-enabled call raises NotImplementedError, as before."""
import torch
import torch.nn as nn

from . import _lib
from .estimator import _param_key


class NativeFp32Module(nn.Module):
    _what = "module"            # for messages
    _engine_kwarg = None        # _lib.Engine keyword selecting the handle kind
    native_training = False     # opt-in: grad-enabled calls train on the native kernels (instance / subclass attribute)

    def __init__(self):
        super().__init__()
        self._engine = None
        self._engine_key = None

    def _native_config(self):  # pragma: no cover
        raise NotImplementedError

    def __getstate__(self):
        st = self.__dict__.copy()      # the ctypes engine handle is per-process, never copied/pickled
        st["_engine"] = None
        st["_engine_key"] = None
        return st

    def sync_weights(self):
        """Force a weight re-upload at the next call (after writes through ``p.data`` that bypass the version counter)."""
        self._engine_key = None

    def _apply(self, fn, *a, **k):
        self._engine_key = None
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        self._engine_key = None
        return super()._load_from_state_dict(*a, **k)

    def engine(self):
        """The native handle bound to the device of the parameters, with weights in sync."""
        p0 = next(self.parameters())
        if p0.device.type != "cuda":
            raise RuntimeError(f"stabletts_amd: the {self._what} runs only on a HIP device (move the module with .to('cuda')); "
                               "there is no CPU fallback")
        dev = p0.device.index if p0.device.index is not None else torch.cuda.current_device()
        if self._engine is None or self._engine.device != dev:
            if self._engine is not None:
                self._engine.close()
            self._engine = _lib.Engine(0, 0, 0, 0, 0, 0, 0, "f16", dev, **{self._engine_kwarg: self._native_config()})
            self._engine_key = None
        key = _param_key(self)
        if self.native_training:
            # bound in place: a new storage (first use, .to(), re-assignment) re-binds; an in-place update needs nothing
            named = list(self.named_parameters())
            if all(p.dtype == torch.float32 and p.is_contiguous() for _, p in named):
                if key[0] != (self._engine_key[0] if self._engine_key else None):
                    with torch.no_grad():
                        self._engine.bind_parameters([(n, p.detach()) for n, p in named])    # st_finalize synchronises once
                self._engine_key = key
                return self._engine
        if key != self._engine_key:
            with torch.no_grad():
                torch.cuda.synchronize(dev)
                self._engine.load_state_dict(self.state_dict())
            self._engine_key = key
        return self._engine

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


def _stale_check(ctx, what):
    mod, eng = ctx.mod, ctx.eng
    if (eng is not mod._engine or eng.handle is None or eng.train_serial() != ctx.serial
            or _param_key(mod)[1] != ctx.vers):
        raise RuntimeError(
            f"stabletts_amd: this backward's activations are gone -- the {what}'s engine keeps the activations of ONE "
            "grad-enabled forward, and another grad-enabled forward, an optimizer step / parameter update or a device move "
            "happened since.  Call backward() before the next grad-enabled forward or parameter update.")


def _param_grads(ctx, eng, flat):
    """Every parameter's gradient as a view of the flat buffer (zeros where due: DDP needs a gradient for each)."""
    lay = eng.grad_layout()
    out = []
    for name, p in zip(ctx.names, ctx.params):
        off, n, _ = lay[name]
        out.append(flat[off:off + n].view(p.shape))
    return out


def _seed(p):
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0.0 else 0


class _StyleEncoderFn(torch.autograd.Function):
    """MelStyleEncoder.forward under autograd: st_style_encoder_train_forward keeps the activations in the engine, the
    backward is st_style_encoder_train_backward.  Inputs (module, names, mel, mask, *parameters); output c.  The mel is data:
    no input gradient."""

    @staticmethod
    def forward(ctx, mod, names, mel, mask, *params):
        eng = mod.engine()
        dev = mel.device
        B, _, T = mel.shape
        c = torch.empty(B, mod.out_dim, device=dev, dtype=torch.float32)
        p_drop = float(mod.dropout) if mod.training else 0.0
        seed = _seed(p_drop)
        with torch.cuda.device(dev):
            eng.style_encoder_train_forward(mel, mask, c, p_drop, seed, torch.cuda.current_stream(dev).cuda_stream)
        ctx.mod, ctx.eng, ctx.serial, ctx.vers = mod, eng, eng.train_serial(), _param_key(mod)[1]
        ctx.names, ctx.params, ctx.shape, ctx.dev = names, params, (B, T), dev
        ctx.set_materialize_grads(False)
        return c

    @staticmethod
    def backward(ctx, grad_c):
        _stale_check(ctx, "style encoder")
        if grad_c is None:
            return (None,) * (4 + len(ctx.params))
        eng, dev = ctx.eng, ctx.dev
        B, T = ctx.shape
        gc = grad_c.detach().to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            flat = torch.zeros(eng.grad_layout()[None], device=dev, dtype=torch.float32)     # (the alignment gaps stay 0)
            eng.style_encoder_train_backward(ctx.serial, B, T, gc, flat, torch.cuda.current_stream(dev).cuda_stream)
        return (None, None, None, None, *_param_grads(ctx, eng, flat))


class _DurationPredictorFn(torch.autograd.Function):
    """DurationPredictor.forward under autograd: st_duration_predictor_train_forward / _backward.  Inputs (module, names, x,
    x_mask, g, *parameters); output logw.  x and g are detached as in the reference: no input gradient."""

    @staticmethod
    def forward(ctx, mod, names, x, x_mask, g, *params):
        eng = mod.engine()
        dev = x.device
        B, _, T = x.shape
        logw = torch.empty(B, 1, T, device=dev, dtype=torch.float32)
        p_drop = float(mod.p_dropout) if mod.training else 0.0
        seed = _seed(p_drop)
        with torch.cuda.device(dev):
            eng.duration_predictor_train_forward(x, x_mask, g, logw, p_drop, seed, torch.cuda.current_stream(dev).cuda_stream)
        ctx.mod, ctx.eng, ctx.serial, ctx.vers = mod, eng, eng.train_serial(), _param_key(mod)[1]
        ctx.names, ctx.params, ctx.shape, ctx.dev = names, params, (B, T), dev
        ctx.set_materialize_grads(False)
        return logw

    @staticmethod
    def backward(ctx, grad_logw):
        _stale_check(ctx, "duration predictor")
        if grad_logw is None:
            return (None,) * (5 + len(ctx.params))
        eng, dev = ctx.eng, ctx.dev
        B, T = ctx.shape
        gl = grad_logw.detach().to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            flat = torch.zeros(eng.grad_layout()[None], device=dev, dtype=torch.float32)
            eng.duration_predictor_train_backward(ctx.serial, B, T, gl, flat, torch.cuda.current_stream(dev).cuda_stream)
        return (None, None, None, None, None, *_param_grads(ctx, eng, flat))
