"""What every module that owns a native handle shares: ``NativeModule`` (the handle's life cycle: created on the parameters'
device, dropped from pickles, re-synchronised when the parameters move or change) and the helpers of their autograd
Functions.  Decoder, TextEncoder, Vocos and the fp32 modules (MelStyleEncoder, DurationPredictor) derive from it."""
import torch
import torch.nn as nn


def _param_key(module):
    """(storage identity, version counters) of the parameters.  The first changes when a tensor moves (``.to()``,
    ``.half()``, re-assignment), the second whenever autograd-visible code rewrites a weight in place (optimizer step,
    ``load_state_dict``).  Inference tensors (a module built or moved under torch.inference_mode) carry no version
    counter; they key on the address alone and need sync_weights() after an in-place update."""
    ptrs, vers = [], []
    for p in module.parameters():
        try:
            ver = p._version
        except RuntimeError:
            ver = -1
        ptrs.append((p.data_ptr(), p.dtype, p.is_contiguous()))
        vers.append(ver)
    return tuple(ptrs), tuple(vers)


def sync_engine_params(module, dev):
    """Brings ``module._engine``'s view of the parameters up to date (the decoder's and the text encoder's sync policy).
    A change of storage (first use, ``.to()``, dtype change) binds the fp32 tensors in place (st_bind_param, or fp32 staging
    copies for a non-fp32 module) and packs the 16-bit copies (st_finalize); an in-place update (optimizer step) only re-packs,
    as kernels on the current stream (st_repack).  Uses / sets ``_engine_key``, ``_engine_vers``, ``_staging``."""
    key, vers = module._param_key()
    if key != module._engine_key:
        with torch.no_grad():
            named = list(module.named_parameters())
            if all(p.dtype == torch.float32 and p.is_contiguous() for _, p in named):
                module._staging = None
                bound = [(n, p.detach()) for n, p in named]
            else:       # e.g. a .half() module: the engine reads fp32 staging copies
                module._staging = [p.detach().to(dtype=torch.float32).contiguous() for _, p in named]
                bound = [(n, s) for (n, _), s in zip(named, module._staging)]
            module._engine.bind_parameters(bound)        # st_finalize synchronises the device: pending writes have landed
        module._engine_key, module._engine_vers = key, vers
    elif vers != module._engine_vers:
        with torch.no_grad(), torch.cuda.device(dev):
            if module._staging is not None:
                for s, p in zip(module._staging, module.parameters()):
                    s.copy_(p)
            module._engine.repack(torch.cuda.current_stream(dev).cuda_stream)
        module._engine_vers = vers


def hip_device_index(device, what):
    """Index of the HIP device ``device``; raises where the `what` sits on anything else (there is no CPU fallback)."""
    if device.type != "cuda":
        raise RuntimeError(f"stabletts_amd: the {what} runs only on a HIP device (move the module with .to('cuda')); "
                           "there is no CPU fallback")
    return device.index if device.index is not None else torch.cuda.current_device()


def host_lengths(lengths, x):
    """The ``lengths`` of a ragged vocoder call (``forward_ragged`` of Vocos and FireflyGANBase) as a list of Python ints: a
    sequence, or a one-dimensional integer tensor on the CPU or on the device of the mel ``x`` (a device tensor costs one
    ``.tolist()`` sync).  Their count and range are checked by the native entry point."""
    if isinstance(lengths, torch.Tensor):
        if lengths.dtype.is_floating_point or lengths.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise ValueError(f"lengths must be an integer tensor, got {lengths.dtype}")
        if lengths.device.type != "cpu" and lengths.device != x.device:
            raise ValueError(f"lengths is on {lengths.device}, the mel is on {x.device}")
        if lengths.dim() != 1:
            raise ValueError("lengths must be one-dimensional (B,)")
        return lengths.tolist()
    return [int(n) for n in lengths]


class NativeModule(nn.Module):
    """A parameter container whose forward runs on a handle of libstabletts_hip.so.  A subclass says how the handle is
    created (``_create_engine``), sets ``_what`` and ``operand_dtype``, and picks one of the two sync policies:
    ``_rebind = True`` binds the parameters in place and re-packs after in-place updates (sync_engine_params);
    ``_rebind = False`` re-loads every parameter when ``_param_key()`` changed."""
    _what = "module"            # the module's noun in messages
    operand_dtype = "f16"       # MFMA operand type of the handle; a handle of another type is stale (the fp32 modules keep this)
    _rebind = True

    def __init__(self):
        super().__init__()
        self._engine = None
        self._engine_key = None        # storage identity of the parameters the engine is bound to (re-load: the whole key)
        self._engine_vers = None       # their version counters at the last (re)pack
        self._staging = None           # fp32 copies the engine reads when the parameters themselves are not fp32

    def __getstate__(self):
        st = self.__dict__.copy()      # the ctypes engine handle is per-process, never copied/pickled
        st["_engine"] = None
        st["_engine_key"] = st["_engine_vers"] = st["_staging"] = None
        return st

    def _apply(self, fn, *a, **k):            # .to() / .cuda() / .half(): storage changes
        self._engine_key = None
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        self._engine_key = None
        return super()._load_from_state_dict(*a, **k)

    def _param_key(self):
        return _param_key(self)

    def sync_weights(self):
        """Force the engine to re-pack its 16-bit weight copies (``_rebind`` modules) or re-load the parameters (the others)
        at the next call.  Needed only after writes that bypass autograd's version counter (``p.data.copy_(ema)``,
        ``m.weight.data.normal_()``, as some EMA / weight-swap utilities do); in-place ops on the parameters themselves,
        optimizer steps, ``load_state_dict`` and ``.to()`` are detected automatically."""
        if self._rebind:
            self._engine_vers = None
        else:
            self._engine_key = None

    def _create_engine(self, dev):  # pragma: no cover
        raise NotImplementedError

    def _sync(self, dev):
        if self._rebind:
            return sync_engine_params(self, dev)
        key = self._param_key()
        if key != self._engine_key:
            with torch.no_grad():
                torch.cuda.synchronize(dev)
                self._engine.load_state_dict(self.state_dict())
            self._engine_key = key

    def engine(self):
        """The native handle bound to the device of the parameters, with weights in sync."""
        dev = hip_device_index(next(self.parameters()).device, self._what)
        if self._engine is None or self._engine.device != dev or self._engine.operand_dtype != self.operand_dtype:
            if self._engine is not None:
                self._engine.close()
            self._engine = self._create_engine(dev)
            self._engine_key = None
        self._sync(dev)
        return self._engine


# ---- helpers of the autograd Functions around the native training entry points
def dropout_seed(p_drop):
    """A fresh 63-bit seed of the counter-based dropout from torch's CPU generator (``torch.manual_seed`` reproduces a run)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if p_drop > 0.0 else 0


def check_activations_live(mod, eng, serial, vers=None, advice="or parameter update."):
    """Raises when the activations of forward `serial` are no longer in the engine (``vers``: the parameters' version counters
    at that forward, for the modules whose engine does not drop the activations on a parameter update by itself)."""
    if (eng is not mod._engine or eng.handle is None or eng.train_serial() != serial
            or (vers is not None and mod._param_key()[1] != vers)):
        raise RuntimeError(
            f"stabletts_amd: this backward's activations are gone -- the {mod._what}'s engine keeps the activations of ONE "
            "grad-enabled forward, and another grad-enabled forward, an optimizer step / parameter update or a device move "
            f"happened since.  Call backward() before the next grad-enabled forward {advice}")


def param_grad_views(flat, lay, names, params, need):
    """Views of the flat gradient buffer the native backward wrote into (no copy): one storage for all parameters of this
    backward, each slice 64-byte aligned; a parameter's .grad keeps that storage alive until it is replaced.  None where
    autograd does not need the gradient."""
    out = []
    for name, p, nd in zip(names, params, need):
        if not nd:
            out.append(None)
            continue
        off, n, _ = lay[name]
        out.append(flat[off:off + n].view(p.shape))
    return out
