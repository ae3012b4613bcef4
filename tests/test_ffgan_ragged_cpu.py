"""What the ragged FireflyGAN entry (FireflyGANBase.forward_ragged / st_ffgan_forward_ragged) promises without a device: the
export, the Python surface, the argument rules that hold before any engine is created, and the lengths helper it shares with
Vocos.forward_ragged.  The arithmetic itself is tested on the GPU (tests/test_gpu_ffgan_ragged.py)."""
import numpy as np
import pytest
import torch

from tests import ffgan_restatement as R


@pytest.fixture(scope="module")
def lib():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def module():
    from stabletts_amd.ffgan import FireflyGANBase
    return FireflyGANBase(config=R.small_config())


def test_library_exports_the_entry_and_rejects_a_null_handle(lib):
    assert lib.st_ffgan_forward_ragged(None, None, None, None, 1, 1, None) == -1      # ST_ERR_INVALID


def test_forward_ragged_is_on_the_module_and_on_the_wrapper(module):
    from stabletts_amd.ffgan import FireflyGANBase, FireflyGANBaseWrapper
    assert callable(FireflyGANBase.forward_ragged) and callable(FireflyGANBaseWrapper.forward_ragged)
    from stabletts_amd._lib import Engine
    assert callable(Engine.ffgan_forward_ragged)


BAD_LENGTHS = {
    "float": (lambda: torch.tensor([4.0, 2.0]), "integer tensor"),
    "bool": (lambda: torch.tensor([True, True]), "integer tensor"),
    "two_dimensional": (lambda: torch.tensor([[4, 2]]), "one-dimensional"),
    "other_device": (lambda: torch.empty(2, dtype=torch.int64, device="meta"), "lengths is on meta"),
}


@pytest.mark.parametrize("case", sorted(BAD_LENGTHS))
def test_bad_lengths_raise_before_any_engine_is_created(module, case):
    make, pattern = BAD_LENGTHS[case]
    mel = torch.zeros(2, 64, 4)
    with pytest.raises(ValueError, match=pattern):
        module.forward_ragged(mel, make())
    assert module._engine is None


def test_a_cpu_mel_raises_before_any_engine_is_created(module):
    with pytest.raises(ValueError, match="no CPU fallback"):
        module.forward_ragged(torch.zeros(2, 64, 4), [4, 2])
    with pytest.raises(ValueError, match="no CPU fallback"):
        module.forward_ragged(torch.zeros(2, 64, 4), torch.tensor([4, 2], dtype=torch.int32))
    assert module._engine is None


def test_lengths_helper_is_shared_and_gives_one_list_for_every_input_kind():
    from stabletts_amd import _native_module, ffgan, vocos
    assert ffgan.host_lengths is _native_module.host_lengths and vocos.host_lengths is _native_module.host_lengths
    x = torch.zeros(3, 64, 9)
    want = [9, 1, 4]
    for lengths in (want, tuple(want), np.array(want), np.array(want, dtype=np.int32), torch.tensor(want),
                    torch.tensor(want, dtype=torch.int32), torch.tensor(want, dtype=torch.uint8)):
        got = _native_module.host_lengths(lengths, x)
        assert got == want and all(type(n) is int for n in got), type(lengths)
