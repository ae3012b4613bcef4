"""CPU-only checks of the opt-in native training of the MelStyleEncoder / DurationPredictor: install(..., "train") registers
subclasses with native_training set and the reference's checkpoint keys, the base classes stay inference-only,
install(reference_encoder=True) is unchanged, and the new C entry points are exported and reject NULL handles."""
import ctypes
import importlib
import sys

import pytest
import torch

NAMES = ("models.flow_matching", "models.reference_encoder", "models.duration_predictor")


def _install(**kw):
    import stabletts_amd
    saved = {k: sys.modules.get(k) for k in NAMES}
    try:
        stabletts_amd.install(**kw)
        return importlib.import_module("models.reference_encoder"), importlib.import_module("models.duration_predictor")
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m


def test_install_train_registers_trainable_subclasses_with_reference_keys():
    from stabletts_amd import duration_predictor, reference_encoder
    rem, dpm = _install(reference_encoder="train", duration_predictor="train")
    assert rem.__name__ == "stabletts_amd.reference_encoder_train" and dpm.__name__ == "stabletts_amd.duration_predictor_train"
    assert rem.MelStyleEncoder.native_training is True and dpm.DurationPredictor.native_training is True
    assert issubclass(rem.MelStyleEncoder, reference_encoder.MelStyleEncoder)
    assert issubclass(dpm.DurationPredictor, duration_predictor.DurationPredictor)
    assert rem.Conv1dGLU is reference_encoder.Conv1dGLU and dpm.duration_loss is duration_predictor.duration_loss
    a = rem.MelStyleEncoder(128, style_vector_dim=256, style_kernel_size=5, dropout=0.25)
    b = reference_encoder.MelStyleEncoder(128, style_vector_dim=256, style_kernel_size=5, dropout=0.25)
    assert {k: v.shape for k, v in a.state_dict().items()} == {k: v.shape for k, v in b.state_dict().items()}
    a.load_state_dict(b.state_dict(), strict=True)
    c = dpm.DurationPredictor(256, 1024, 3, 0.5, 256)
    d = duration_predictor.DurationPredictor(256, 1024, 3, 0.5, 256)
    assert {k: v.shape for k, v in c.state_dict().items()} == {k: v.shape for k, v in d.state_dict().items()}
    assert "native_training" not in a.state_dict() and "native_training" not in c.state_dict()


def test_base_classes_stay_inference_only():
    from stabletts_amd.duration_predictor import DurationPredictor
    from stabletts_amd.reference_encoder import MelStyleEncoder
    _install(reference_encoder="train", duration_predictor="train")
    assert MelStyleEncoder.native_training is False and DurationPredictor.native_training is False
    rem, dpm = _install(reference_encoder=True, duration_predictor=True)
    assert rem.__name__ == "stabletts_amd.reference_encoder" and dpm.__name__ == "stabletts_amd.duration_predictor"
    assert rem.MelStyleEncoder is MelStyleEncoder and dpm.DurationPredictor is DurationPredictor


def test_cpu_module_has_no_fallback_with_or_without_training():
    from stabletts_amd.reference_encoder_train import MelStyleEncoder
    m = MelStyleEncoder(128, style_vector_dim=256, style_kernel_size=5, dropout=0.25).train()
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        m(torch.randn(2, 128, 9))
    with torch.no_grad(), pytest.raises(RuntimeError, match="runs only on a HIP device"):
        m(torch.randn(2, 128, 9))


def test_training_symbols_are_exported_and_reject_null():
    from stabletts_amd import _lib
    from stabletts_amd.build import build
    build(verbose=False)
    names = ("st_style_encoder_train_forward", "st_style_encoder_train_backward", "st_duration_predictor_train_forward",
             "st_duration_predictor_train_backward")
    assert all(n in _lib.EXPORTS for n in names)
    lib = _lib.load()
    assert lib.st_abi_version() == 4
    assert lib.st_style_encoder_train_forward.argtypes[-3:] == [ctypes.c_float, ctypes.c_uint64, ctypes.c_void_p]
    assert lib.st_duration_predictor_train_forward.argtypes[-3:] == [ctypes.c_float, ctypes.c_uint64, ctypes.c_void_p]
    assert lib.st_style_encoder_train_forward(None, None, None, None, 1, 1, 0.0, 0, None) == -1
    assert lib.st_style_encoder_train_backward(None, 1, 1, 1, None, None, None) == -1
    assert lib.st_duration_predictor_train_forward(None, None, None, None, None, 1, 1, 0.0, 0, None) == -1
    assert lib.st_duration_predictor_train_backward(None, 1, 1, 1, None, None, None) == -1
    assert lib.st_train_serial(None) == 0
