"""CPU-only checks of the text encoder's training path: the shim refuses a CPU module with the usual message (no fallback,
with or without autograd), and the library exports the two training entry points with the declared argument types."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_training_path_on_a_cpu_module_fails_with_the_hip_device_message():
    from stabletts_amd.text_encoder import TextEncoder
    m = TextEncoder(401, 128, 256, 1024, 4, 3, 3, 0.1, 256).train()
    tok = torch.zeros(2, 9, dtype=torch.long)
    c = torch.randn(2, 256, requires_grad=True)
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        m(tok, c, torch.tensor([9, 4]))
    with torch.no_grad(), pytest.raises(RuntimeError, match="runs only on a HIP device"):
        m(tok, c, torch.tensor([9, 4]))


def test_training_symbols_are_exported():
    import ctypes
    from stabletts_amd import _lib
    for name in ("st_text_encoder_train_forward", "st_text_encoder_train_backward"):
        assert name in _lib.EXPORTS
    lib = _lib.load()
    assert lib.st_abi_version() == 4
    assert lib.st_text_encoder_train_forward.argtypes[-3:] == [ctypes.c_float, ctypes.c_uint64, ctypes.c_void_p]
    assert len(lib.st_text_encoder_train_backward.argtypes) == 9
    # a NULL handle is rejected before anything touches a device
    assert lib.st_text_encoder_train_backward(None, 1, 1, 1, None, None, None, None, None) < 0
    assert lib.st_train_param_part(None, b"emb.weight") < 0
