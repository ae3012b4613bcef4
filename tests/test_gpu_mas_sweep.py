"""mas_path_kernel on every register plan (K = 1 ... 64 groups of 64 columns) with both decision-bit stores (LDS, global
workspace), 14 instantiations, against the numpy restatement (tests/mas_restatement.py) on the cases of tests/align_sweep_cases.py
-- bitwise.  Also: the exact LDS budget on both sides with one input, row counts around the prefetch ring and the 64-row backtrack
window, ties past the first group, the forced diagonal across two word boundaries, NaN in every cell the kernel says it never
uses, an item alone against the item in its batch, and the fused neg_cent with Tx on a tile edge and one past it.
tests/test_align_sweep_cpu.py states what the inputs are.  Run with ``-m gpu``.

Measured on an MI355X (profiles/align_sweep_parity.txt): see MEASURED below.
"""
import numpy as np
import pytest
import torch

from tests import align_sweep_cases as sc
from tests import test_gpu_mas as tgm

pytestmark = pytest.mark.gpu

# MEASURED (MI355X, profiles/align_sweep_parity.txt): the 19 table rows, the three row-edge cases, the ties case and the diagonal
# give 0 cells that differ from the restatement's path; word crossings per case 0 at K = 1 and at 2 x 1025, otherwise 1 - 14 (the ones
# tests/test_align_sweep_cpu.py prints); this file and tests/test_gpu_align_sweep.py together take 2.8 s, the slowest case 0.25 s.
# A scratch build whose launcher sent two groups to the K = 1 plan passed every earlier test and failed six tests here.


def native(nc, t_y, t_x):
    from stabletts_amd.alignment import maximum_path
    path, dur = maximum_path(torch.tensor(nc).cuda(), torch.tensor(t_y), torch.tensor(t_x), durations=True)     # (copies: the cases are read-only)
    assert path.dtype == torch.float32 and dur.dtype == torch.int32
    return path.cpu().numpy(), dur.cpu().numpy()


def check_case(label, case, ref):
    """Bitwise the restatement, the structure of tests/test_gpu_mas.py, durations = column sums (0 behind t_x), two runs equal."""
    nc, t_y, t_x = case
    path, dur = native(nc, t_y, t_x)
    B, Ty, Tx = nc.shape
    crossings = sum(sc.word_crossings(ref[b], t_y[b]) for b in range(B))
    print(f"mas_sweep {label:<24} plan K={sc.plan_of(Tx)} (ring {sc.RING[sc.plan_of(Tx)]}) store {sc.store_of(Ty, Tx):<6} "
          f"B={B} word crossings {crossings}  mismatching cells {int((path != ref).sum())}")
    assert np.array_equal(path, ref.astype(np.float32))
    tgm._check_structure(path, dur, t_y, t_x)
    assert np.array_equal(dur, path.sum(1).astype(np.int32))
    for b in range(B):
        assert not dur[b, int(t_x[b]):].any()
    again, dur2 = native(nc, t_y, t_x)
    assert np.array_equal(again, path) and np.array_equal(dur2, dur)
    return path, dur


@pytest.mark.parametrize("row", sc.MAS_TABLE, ids=sc.mas_id)
def test_table_row_is_bitwise_the_restatement(row):
    check_case(sc.mas_id(row), sc.mas_case(*row), sc.mas_reference(row))


@pytest.mark.parametrize("name", list(sc.mas_extra_cases()))
def test_row_edges_ties_and_diagonal(name):
    path, _ = check_case(name, sc.mas_extra_cases()[name](), sc.mas_reference(name))
    if name == "diagonal":
        assert np.array_equal(path[0], np.eye(130, dtype=np.float32))


@pytest.mark.parametrize("row", sc.POISON_ROWS, ids=sc.mas_id)
def test_cells_outside_an_item_are_never_used(row):
    """NaN in every cell outside [0, t_y) x [0, t_x): a NaN that reached a compare or an add would move a decision bit or a path."""
    nc, t_y, t_x = sc.mas_case(*row)
    bad = sc.poisoned(nc, t_y, t_x)
    assert np.isnan(bad).any()
    clean, poisoned = native(nc, t_y, t_x), native(bad, t_y, t_x)
    assert np.array_equal(poisoned[0], clean[0]) and np.array_equal(poisoned[1], clean[1])
    assert np.array_equal(poisoned[0], sc.mas_reference(row).astype(np.float32))


@pytest.mark.parametrize("row", sc.ALONE_ROWS, ids=sc.mas_id)
def test_an_item_alone_equals_the_item_in_the_batch(row):
    nc, t_y, t_x = sc.mas_case(*row)
    whole = native(nc, t_y, t_x)
    for b in range(nc.shape[0]):
        alone = native(nc[b:b + 1], t_y[b:b + 1], t_x[b:b + 1])               # the same Ty and Tx: the same plan and store
        assert np.array_equal(alone[0][0], whole[0][b]) and np.array_equal(alone[1][0], whole[1][b]), b


def test_both_sides_of_the_lds_budget_give_one_path():
    """4096 x 2 words x 8 B is the whole budget, one row more goes to the global workspace: with t_y <= 4096 on both tensors and
    the same first 4096 rows the two kernels must agree."""
    from stabletts_amd import _lib
    lib = _lib.load()
    assert lib.st_maximum_path_workspace_bytes(3, 4096, 128) == 0 and lib.st_maximum_path_workspace_bytes(3, 4097, 128) > 0
    small, t_y, t_x = sc.mas_case(4096, 128)
    big = sc.mas_case(4097, 128)[0]
    in_lds, in_global = native(small, t_y, t_x), native(big, t_y, t_x)
    assert np.array_equal(in_global[0][:, :4096], in_lds[0]) and not in_global[0][:, 4096:].any()
    assert np.array_equal(in_global[1], in_lds[1])
    assert np.array_equal(in_lds[0], sc.mas_reference((4096, 128)).astype(np.float32))


@pytest.mark.parametrize("B,D,Tx,Ty", [(2, 80, 65, 129), (2, 17, 64, 64)])
def test_fused_neg_cent_on_a_tile_edge(B, D, Tx, Ty):
    """Tx exactly one 64-token tile and one token past it, D no multiple of the 16-channel chunk: the gate of
    tests/test_gpu_mas.py::test_fused_neg_cent_against_fp64 (1e-5 of max |neg_cent| against float64)."""
    tgm.test_fused_neg_cent_against_fp64(B, D, Tx, Ty)
