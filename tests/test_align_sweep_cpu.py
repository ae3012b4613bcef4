"""The alignment sweep on a CPU-only box: the conditions on the inputs that tests/test_gpu_mas_sweep.py and
tests/test_gpu_align_sweep.py rely on.  The table of tests/align_sweep_cases.py reaches all 14 (register plan, decision-bit store)
instantiations of mas_path_kernel, with the store restated from the launcher's rule and checked against the library's own host
function; the rows said to sit on the LDS budget do; every plan above one group has a path that crosses a 64-column word; the
ties case has ties; the aligned-loss cases hold what they claim (scan chunks above one, a token across frame blocks, a token
without frames on a chunk edge, malformed counts in a chunk's second token, grids past their caps); the length-regulation
restatement (tests/align_restatement.py) reproduces the committed reference fixture bit for bit, and its new inputs keep
exp(logw) away from the integers."""
import os
import time

import numpy as np
import pytest
import torch

from oracle.make_golden_align import CASES as GOLDEN_REGULATE_CASES, align_inputs
from tests import align_loss_restatement as ar
from tests import align_restatement as lr
from tests import align_sweep_cases as sc
from tests import mas_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from stabletts_amd.build import build
    build(verbose=False)
    from stabletts_amd import _lib
    return _lib.load()


def test_plan_rule():
    assert [sc.plan_of(tx) for tx in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert set(sc.RING) == set(sc.PLANS) and all(k * sc.RING[k] <= 64 or sc.RING[k] == 2 for k in sc.PLANS if k >= 8)


def test_table_covers_every_plan_and_store(lib):
    seen = {(sc.plan_of(Tx), sc.store_of(Ty, Tx)) for Ty, Tx in sc.MAS_TABLE}
    assert seen == {(k, s) for k in sc.PLANS for s in ("lds", "global")}
    for Ty, Tx in sc.MAS_TABLE:
        in_lds = lib.st_maximum_path_workspace_bytes(3, Ty, Tx) == 0
        assert in_lds == (sc.store_of(Ty, Tx) == "lds"), (Ty, Tx)
        if not in_lds:
            assert lib.st_maximum_path_workspace_bytes(3, Ty, Tx) == 3 * sc.bits_bytes(Ty, Tx)
    for rows, store in ((sc.POISON_ROWS, None), (sc.ALONE_ROWS, "global")):
        assert set(rows) <= set(sc.MAS_TABLE)
        assert store is None or all(sc.store_of(*r) == store for r in rows)
    assert sorted((sc.plan_of(Tx), sc.store_of(Ty, Tx)) for Ty, Tx in sc.POISON_ROWS) == sorted(seen)    # one of each
    assert [sc.plan_of(Tx) for _, Tx in sc.ALONE_ROWS] == [4, 16, 64]
    for Tx in sc.ROW_EDGE_WIDTHS:
        assert sc.store_of(65, Tx) == "lds"
    assert [sc.RING[sc.plan_of(Tx)] for Tx in sc.ROW_EDGE_WIDTHS] == [16, 4, 2]


def test_rows_on_the_budget_are_on_it(lib):
    for Ty, Tx in sc.ON_THE_BUDGET:
        assert (Ty, Tx) in sc.MAS_TABLE and sc.bits_bytes(Ty, Tx) == sc.LDS_BUDGET and sc.store_of(Ty, Tx) == "lds"
        assert (Ty + 1, Tx) in sc.MAS_TABLE and sc.store_of(Ty + 1, Tx) == "global"
        assert lib.st_maximum_path_workspace_bytes(1, Ty, Tx) == 0 and lib.st_maximum_path_workspace_bytes(1, Ty + 1, Tx) > 0
    small, big = sc.mas_case(4096, 128), sc.mas_case(4097, 128)
    assert np.array_equal(small[0], big[0][:, :4096])                 # the budget-boundary test runs both kernels on one input


def test_case_lengths():
    for Ty, Tx in sc.MAS_TABLE:
        nc, t_y, t_x = sc.mas_case(Ty, Tx)
        assert nc.shape == (3, Ty, Tx) and nc.dtype == np.float32
        assert t_y.tolist() == [Ty, max(Ty - 1, 1), Ty // 2 + 1] and t_x.tolist() == [Tx, max(Tx - 1, 1), min(37, Tx)]
        assert t_x[2] <= 64                                            # only group 0
    for Tx in sc.ROW_EDGE_WIDTHS:
        nc, t_y, t_x = sc.row_edge_case(Tx)
        assert nc.shape == (9, 65, Tx) and t_y.tolist() == [1, 2, 3, 15, 16, 17, 63, 64, 65]
        assert t_x.tolist() == [1, 1, 3, 14, 16, 16, 63, 63, 65]
    nc, t_y, t_x = sc.diagonal_case()
    assert nc.shape == (1, 130, 130) and t_y[0] == t_x[0] == 130


def test_word_crossings_helper():
    path = np.zeros((5, 130), np.int32)
    path[np.arange(5), [62, 63, 64, 64, 65]] = 1
    assert sc.word_crossings(path, 5) == 1 and sc.word_crossings(path, 2) == 0
    path = np.zeros((3, 130), np.int32)
    path[np.arange(3), [127, 128, 129]] = 1
    assert sc.word_crossings(path, 3) == 1


def test_restatement_sweep_is_cheap_and_crosses_words():
    """The whole restatement side of the search: every table row and extra case, timed; summed over the restatement's paths every
    plan with K >= 2 has a step from column 64 k to 64 k - 1, the diagonal crosses two."""
    start = time.perf_counter()
    crossings = {k: 0 for k in sc.PLANS}
    for Ty, Tx in sc.MAS_TABLE:
        _, t_y, _ = sc.mas_case(Ty, Tx)
        ref = sc.mas_reference((Ty, Tx))
        n = sum(sc.word_crossings(ref[b], t_y[b]) for b in range(3))
        crossings[sc.plan_of(Tx)] += n
        print(f"{sc.mas_id((Ty, Tx))}: {n} word crossings")
    for name, case in sc.mas_extra_cases().items():
        _, t_y, _ = case()
        ref = sc.mas_reference(name)
        print(f"{name}: {sum(sc.word_crossings(ref[b], t_y[b]) for b in range(len(t_y)))} word crossings")
    took = time.perf_counter() - start
    print(f"restatement sweep: {took:.2f} s")
    assert took < 20                                                   # (under 1 s where it was written)
    assert crossings[1] == 0 and all(crossings[k] >= 1 for k in sc.PLANS if k >= 2), crossings
    assert sc.word_crossings(sc.mas_reference("diagonal")[0], 130) == 2
    cols = sc.mas_reference("diagonal")[0].argmax(1)
    assert np.array_equal(cols, np.arange(130))


def test_ties_case_has_ties_past_the_first_group():
    """The criterion of tests/test_mas_cpu.py::test_ties_case_has_ties, on the columns the first group does not hold."""
    nc, t_y, t_x = sc.ties_case()
    assert set(np.unique(nc)) == {-1.0, 0.0, 1.0}
    for b in range(2):
        tx = int(t_x[b])
        v = mr.dp_values(nc[b].copy(), int(t_y[b]), tx)
        ties = (v[:, 1:tx] == v[:, :tx - 1])
        assert ties.sum() > 50 and ties[:, 64:].sum() > 50, (ties.sum(), ties[:, 64:].sum())


def test_poisoned_cells_are_outside_every_item():
    nc, t_y, t_x = sc.mas_case(130, 129)
    p = sc.poisoned(nc, t_y, t_x)
    assert np.isfinite(p[0]).all() and np.isnan(p[1, 129:]).all() and np.isnan(p[1, :, 128:]).all() and np.isnan(p[2, :, 37:]).all()
    assert np.array_equal(p[1, :129, :128], nc[1, :129, :128]) and np.array_equal(p[2, :66, :37], nc[2, :66, :37])


# ---- the aligned losses
@pytest.mark.parametrize("shape", list(sc.SCAN_CASES), ids=sc.scan_id)
def test_scan_cases_are_what_they_claim(shape):
    B, M, Tx, Ty = shape
    g = sc.scan_case(shape)
    assert g["mu_x"].shape == (B, M, Tx) and g["y"].shape == (B, M, Ty) and g["durations"].shape == (B, Tx)
    assert g["x_lengths"].max() == Tx and (B == 1 or len(set(g["x_lengths"])) == B)                # ragged
    assert (g["durations"].sum(1) == g["y_lengths"]).all() and (g["durations"] >= 0).all()
    assert B == 1 or (g["keep"].any() and not g["keep"].all())
    assert np.abs(g["fake_content"]).min() > 0
    assert sc.zero_token_on_a_chunk_edge(g)
    if Ty > 256:
        assert g["durations"].max() > 256                              # one token spans frame blocks of the forward
    assert sc.scan_chunk(Tx) == {64: 1, 65: 1, 256: 1, 257: 2, 350: 2, 4096: 16}[Tx]
    f, r = sc.restated(("scan", shape))
    assert np.array_equal(r["n"].sum(1), g["y_lengths"]) and f["frame_token"].max() == Tx - 1


def test_scan_cases_cover_the_issue():
    chunks = {sc.scan_chunk(s[2]) for s in sc.SCAN_CASES}
    assert chunks == {1, 2, 16}
    assert any(s[2] > 64 for s in sc.SCAN_CASES)                       # the backward's second token block
    assert {s[1] % 16 for s in sc.SCAN_CASES} >= {1, 3, 0}             # a last channel block with fewer channels than waves
    assert max(s[2] for s in sc.SCAN_CASES) == 4096                    # the kernels' limit


def test_malformed_case_is_malformed_in_the_second_token_of_a_chunk():
    g = sc.scan_case(sc.MALFORMED_SHAPE)
    Ty = g["y"].shape[2]
    both, only1 = sc.malformed_durations(g)
    assert both[0].sum() > Ty and np.array_equal(both[1], only1[1]) and np.array_equal(only1[0], g["durations"][0])
    assert only1[1, 55] < 0 and g["x_mask"][1, 0, 55] == 1 and 55 % 2 == 1
    assert only1[1, 201] > 0 and g["x_mask"][1, 0, 201] == 0 and 201 % 2 == 1
    ends = ar.segment_ends(both, g["x_mask"], Ty)
    assert ends.max() == Ty and ends[0, -1] == Ty and ends[1, 55] == ends[1, 54] and ends[1, 201] == ends[1, 200]
    assert g["durations"][1, 55] > 0                                    # the negative count takes frames away


@pytest.mark.parametrize("B,Tx", sc.DUR_GRID_SHAPES)
def test_duration_grid_cases_pass_the_grid_caps(B, Tx):
    g = sc.duration_grid_case(B, Tx)
    assert B * Tx > {17: 256 * 256, 65: 1024 * 256}[B]                  # blocks x threads of the capped grid
    assert g["y"].shape == (B, 1, 8) and (g["durations"].sum(1) <= 8).all() and (g["durations"] >= 0).all()
    assert g["durations"].sum(1).max() == 8 and (g["durations"] > 0).sum() > B
    assert g["x_lengths"][0] == Tx and g["x_lengths"].min() == 1
    assert (g["logw"] != 0).all()
    _, r = sc.restated(("grid", (B, Tx)))
    assert (r["grad_logw"] != 0).all()


def test_chain_case():
    g = sc.case_by_key(("chain",))
    assert g["mu_x"].shape == sc.CHAIN_SHAPE[:3] and g["y"].shape[2] == 700
    assert g["x_lengths"].tolist() == [300, 211, 1] and g["y_lengths"].tolist() == [655, 700, 9]


# ---- length regulation
@pytest.mark.parametrize("name", list(GOLDEN_REGULATE_CASES))
def test_regulation_restatement_reproduces_the_reference_fixture(name):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "align_outputs.npz"))
    B, Tx, xl, M, ls, seed = GOLDEN_REGULATE_CASES[name]
    logw, mu_x, x_mask, _ = align_inputs(B, Tx, xl, M, seed)
    r = lr.length_regulate(logw, x_mask, mu_x, ls)
    assert np.array_equal(r["w_ceil"].numpy(), gold[name + "_w_ceil"])
    assert np.array_equal(r["y_lengths"].numpy(), gold[name + "_y_lengths"])
    assert np.array_equal(r["y_mask"].numpy(), gold[name + "_y_mask"])
    assert np.array_equal(r["attn"].numpy().astype(np.uint8), gold[name + "_attn"])
    assert r["mu_y"].dtype == torch.float32 and np.array_equal(r["mu_y"].numpy(), gold[name + "_mu_y"])
    attn_mask = x_mask[:, 0, :, None] * r["y_mask"][:, 0, None, :]
    path = lr.generate_path(torch.from_numpy(gold[name + "_w_ceil"])[:, 0], attn_mask)
    assert np.array_equal(path.numpy().astype(np.uint8), gold[name + "_attn"])


@pytest.mark.parametrize("name", list(sc.REGULATE_CASES))
def test_regulation_inputs_keep_away_from_the_integers(name):
    B, Tx, xl, M, ls, seed = sc.REGULATE_CASES[name]
    logw, mu_x, x_mask, lens = align_inputs(B, Tx, xl, M, seed)
    margin = lr.margin_from_integers(logw, x_mask)
    print(f"{name}: exp(logw) is at least {margin:.3g} (relative) from an integer")
    assert margin >= 1e-5
    assert Tx >= 256 and min(xl) == 1 and max(xl) == Tx and len(xl) == B     # ragged, with a one-token utterance
    r = lr.length_regulate(logw, x_mask, mu_x, ls)
    assert r["attn"].shape[1] == Tx and int(r["y_lengths"].max()) == r["attn"].shape[2] > 256
