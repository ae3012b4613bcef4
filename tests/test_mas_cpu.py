"""Monotonic alignment search on a CPU-only box: the numpy restatement (tests/mas_restatement.py) reproduces every path of
tests/golden/mas_outputs.npz (the REAL reference monotonic_align, tools/make_golden_mas.py) exactly; install(monotonic_align=True)
makes models/model.py:5's ``import monotonic_align`` resolve to the drop-in and the registration can be undone; the drop-in
has no CPU fallback; the C entry points reject bad arguments on the host, before any launch."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import mas_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mas_outputs.npz")
CASES = ("ragged", "ties", "equal", "wide", "tx1", "ty1", "single", "clear")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def lib():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    return _lib.load()


def test_fixture_covers_every_case(gold):
    assert {k.split("/")[0] for k in gold} == set(CASES)
    t_y, t_x = mr.lengths_from_mask(gold["wide/mask"])
    assert (t_x > t_y).all()
    assert (mr.lengths_from_mask(gold["tx1/mask"])[1] == 1).all() and (mr.lengths_from_mask(gold["ty1/mask"])[0] == 1).all()
    assert gold["single/neg_cent"].shape[0] == 1
    t_y, t_x = mr.lengths_from_mask(gold["equal/mask"])
    assert (t_x == t_y).all()


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference_paths(gold, case):
    t_y, t_x = mr.lengths_from_mask(gold[case + "/mask"])
    path = mr.maximum_path(gold[case + "/neg_cent"], t_y, t_x)
    assert np.array_equal(path.astype(np.float32), gold[case + "/path"])


def test_ties_case_has_ties(gold):
    """The tie-heavy case is what it claims: equal neighbours in the accumulated rows the backtrack compares."""
    nc = gold["ties/neg_cent"]
    t_y, t_x = mr.lengths_from_mask(gold["ties/mask"])
    v = mr.dp_values(nc[0].copy(), int(t_y[0]), int(t_x[0]))
    ties = (v[:, 1:int(t_x[0])] == v[:, :int(t_x[0]) - 1]).sum()
    assert ties > 50, ties


def test_install_registers_and_restores_monotonic_align():
    import stabletts_amd
    names = ("models.flow_matching", "monotonic_align")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        sys.modules.pop("monotonic_align", None)
        stabletts_amd.install()
        assert "monotonic_align" not in sys.modules
        stabletts_amd.install(monotonic_align=True)
        ma = importlib.import_module("monotonic_align")
        assert ma.__name__ == "stabletts_amd.monotonic_align" and ma.maximum_path is stabletts_amd.maximum_path
        from monotonic_align import maximum_path       # models/model.py:5 then calls monotonic_align.maximum_path
        assert maximum_path is ma.maximum_path
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m
    assert sys.modules.get("monotonic_align") is saved["monotonic_align"]


def test_dropin_raises_on_cpu_tensors():
    from stabletts_amd import alignment, monotonic_align
    nc, mask = torch.zeros(1, 4, 3), torch.ones(1, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        monotonic_align.maximum_path(nc, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        alignment.monotonic_alignment(torch.zeros(1, 2, 3), torch.ones(1, 1, 3), torch.zeros(1, 2, 4), torch.ones(1, 1, 4))


def test_c_entry_points_reject_on_the_host(lib):
    bogus = ctypes.c_void_p(16)          # never dereferenced: every case below returns before any launch
    assert lib.st_maximum_path(None, bogus, bogus, 1, 4, 4, bogus, None, None, None) == -1
    assert lib.st_maximum_path(bogus, bogus, bogus, 0, 4, 4, bogus, None, None, None) == -1
    assert lib.st_maximum_path(bogus, bogus, bogus, 1, 4, 4097, bogus, None, None, None) == -4       # ST_ERR_UNSUPPORTED
    assert "4096" in lib.st_last_error(None).decode()
    assert lib.st_maximum_path(bogus, bogus, bogus, 2, 6000, 700, bogus, None, None, None) == -1     # needs a workspace
    assert "workspace" in lib.st_last_error(None).decode()
    assert lib.st_mas_neg_cent(None, bogus, 1, 80, 4, 4, bogus, None) == -1
    assert lib.st_mas_neg_cent(bogus, bogus, 1, 0, 4, 4, bogus, None) == -1


def test_workspace_bytes(lib):
    assert lib.st_maximum_path_workspace_bytes(64, 1000, 350) == 0                  # 1000 x 6 words x 8 B = 48 KB: LDS
    assert lib.st_maximum_path_workspace_bytes(64, 1024, 512) == 0                  # exactly 64 KiB
    assert lib.st_maximum_path_workspace_bytes(64, 1025, 512) == 64 * 1025 * 8 * 8
    assert lib.st_maximum_path_workspace_bytes(2, 6000, 700) == 2 * 6000 * 11 * 8
    assert lib.st_maximum_path_workspace_bytes(0, 10, 10) == 0
