"""Shared plumbing of the native fp32 modules (MelStyleEncoder, DurationPredictor): a parameter container whose forward runs
in libstabletts_hip.so.  The handle is created on the parameters' device and re-reads the weights whenever their storage or
version counters change, as text_encoder.TextEncoder does.  There is no CPU fallback and no backward."""
import torch
import torch.nn as nn

from . import _lib
from .estimator import _param_key


class NativeFp32Module(nn.Module):
    _what = "module"            # for messages
    _engine_kwarg = None        # _lib.Engine keyword selecting the handle kind

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
        if key != self._engine_key:
            with torch.no_grad():
                torch.cuda.synchronize(dev)
                self._engine.load_state_dict(self.state_dict())
            self._engine_key = key
        return self._engine

    def _check_call(self, tensors):
        """Raises before any work: grad-enabled calls that would need a backward, tensors off the parameters' device."""
        if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors if t is not None)
                                        or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(f"the native {self._what} is inference-only (no backward kernels): call it under "
                                      "torch.no_grad(), or train with the reference module and load its checkpoint")
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            self.engine()      # raises: no CPU fallback
        for t in tensors:
            if t is not None and t.device != dev:
                raise ValueError(f"an input is on {t.device}, the {self._what}'s parameters are on {dev}")
        return dev
