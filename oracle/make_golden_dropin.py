"""Generates tests/golden/stabletts_layout.npz: the checkpoint key layout (state_dict names and shapes) and the decoder's
sigma_min of the REAL reference model, ``StableTTS(401, 128, 256, 1024, 4, 3, 6, 3, 0.1, 256)`` built by the reference's own
models/model.py (imported unmodified, never copied) with all-reference modules.  Before writing, it builds the same model
again after ``stabletts_amd.install(text_encoder=True)`` and checks that models/model.py picks up the native CFMDecoder /
TextEncoder and that the reference's state_dict loads into it strictly.  tests/test_dropin_reference.py then checks the
native modules against the stored layout without the reference.

Only import stand-ins are used for packages absent offline: numba (monotonic_align's decorator) and torchdiffeq.

Run where a checkout of the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python -m oracle.make_golden_dropin
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "stabletts_layout.npz")
MODEL_ARGS = (401, 128, 256, 1024, 4, 3, 6, 3, 0.1, 256)     # n_vocab, mel, hidden, filter, heads, enc layers, dec layers, kernel, p_dropout, gin


def _install_standins():
    class _Ty:                                                  # numba.int32[:, :, ::1] etc. in the signature
        def __getitem__(self, item):
            return self

        def __call__(self, *a, **k):
            return self

    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (lambda f: f)                  # monotonic_align/core.py decorator (training only)
    numba.void = numba.int32 = numba.float32 = _Ty()
    tde = types.ModuleType("torchdiffeq")
    tde.odeint = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("stand-in"))
    sys.modules["numba"] = numba
    sys.modules["torchdiffeq"] = tde


def _purge():
    for k in [k for k in sys.modules if k.split(".")[0] in ("models", "monotonic_align", "utils")]:
        del sys.modules[k]


def _build(native):
    """-> StableTTS instance built by the reference's own models/model.py."""
    import stabletts_amd
    _purge()
    if native:
        stabletts_amd.install(text_encoder=True)
    return importlib.import_module("models.model").StableTTS(*MODEL_ARGS)


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE")
    if not ref_dir or not os.path.isdir(os.path.join(ref_dir, "models")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, ref_dir)
    _install_standins()
    ref = _build(native=False)
    assert type(ref.decoder).__module__ == "models.flow_matching"
    nat = _build(native=True)
    assert type(nat.decoder).__module__ == "stabletts_amd.flow_matching"
    assert type(nat.encoder).__module__ == "stabletts_amd.text_encoder"
    ref_sd = ref.state_dict()
    assert {k: tuple(v.shape) for k, v in nat.state_dict().items()} == {k: tuple(v.shape) for k, v in ref_sd.items()}
    missing, unexpected = nat.load_state_dict(ref_sd, strict=True)
    assert not missing and not unexpected
    assert nat.decoder.sigma_min == ref.decoder.sigma_min
    _purge()
    out = {"state_dict.names": np.array(list(ref_sd.keys())),
           "state_dict.shapes": np.array([",".join(map(str, v.shape)) for v in ref_sd.values()]),
           "decoder.sigma_min": np.array(ref.decoder.sigma_min, dtype=np.float64),
           "model_args": np.array(MODEL_ARGS, dtype=np.float64)}
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, f"({len(ref_sd)} state_dict entries)")


if __name__ == "__main__":
    main()
