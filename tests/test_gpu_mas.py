"""Monotonic alignment search on gfx950 against the REAL reference (tests/golden/mas_outputs.npz, tools/make_golden_mas.py)
and, at shapes the pure-Python reference cannot sweep, against the numpy restatement (tests/mas_restatement.py) on the same
neg_cent.  Paths are compared exactly; neg_cent within 1e-5 of max|neg_cent| of an fp64 computation.  Run with ``-m gpu``."""
import math
import os

import numpy as np
import pytest
import torch

from tests import mas_restatement as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("ragged", "ties", "equal", "wide", "tx1", "ty1", "single", "clear")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mas_outputs.npz")))


def _lengths(B, lo, hi, gen):
    return torch.randint(lo, hi + 1, (B,), generator=gen)


def _neg_cent(B, D, Ty, Tx, t_y, t_x, seed):
    """A training-like neg_cent computed by torch on the GPU (models/model.py:150-155's terms), masked lengths."""
    gen = torch.Generator().manual_seed(seed)
    mu_x = torch.randn(B, D, Tx, generator=gen).cuda()
    y = torch.randn(B, D, Ty, generator=gen).cuda()
    nc = (-0.5 * math.log(2 * math.pi) * D - 0.5 * (y ** 2).sum(1)[:, :, None] + torch.einsum("bdt,bds->bts", y, mu_x)
          - 0.5 * (mu_x ** 2).sum(1)[:, None, :])
    mask = ((torch.arange(Ty)[None, :, None] < t_y[:, None, None]) & (torch.arange(Tx)[None, None, :] < t_x[:, None, None]))
    return nc.contiguous(), mask.float().cuda()


def _check_structure(path, dur, t_y, t_x):
    B, Ty, Tx = path.shape
    for b in range(B):
        ty, tx = int(t_y[b]), int(t_x[b])
        p = path[b]
        assert (p[ty:] == 0).all() and (p[:, tx:] == 0).all()
        assert (p[:ty].sum(1) == 1).all()                         # exactly one 1 per valid row
        cols = p[:ty].argmax(1)
        step = np.diff(cols)
        assert ((step == 0) | (step == 1)).all()                  # monotone, one token at a time
        if tx <= ty:
            assert cols[0] == 0 and cols[-1] == tx - 1
        assert dur[b].sum() == ty and np.array_equal(dur[b], p.sum(0))


@pytest.mark.parametrize("case", CASES)
def test_maximum_path_matches_reference_fixture(gold, case):
    from stabletts_amd.monotonic_align import maximum_path
    nc = torch.from_numpy(gold[case + "/neg_cent"]).cuda()
    mask = torch.from_numpy(gold[case + "/mask"]).cuda()
    path = maximum_path(nc, mask)
    assert path.dtype == torch.float32 and path.device == nc.device
    assert torch.equal(path.cpu(), torch.from_numpy(gold[case + "/path"]))


def test_config5_scale_bitwise_against_restatement():
    from stabletts_amd.alignment import maximum_path
    gen = torch.Generator().manual_seed(5)
    B = 64
    t_y, t_x = _lengths(B, 600, 1000, gen), _lengths(B, 100, 350, gen)
    nc, mask = _neg_cent(B, 80, int(t_y.max()), int(t_x.max()), t_y, t_x, seed=55)
    path, dur = maximum_path(nc, mask.sum(1)[:, 0], mask.sum(2)[:, 0], durations=True)
    ref = mr.maximum_path(nc.cpu().numpy(), t_y.numpy(), t_x.numpy())
    got = path.cpu().numpy()
    assert np.array_equal(got, ref.astype(np.float32))
    _check_structure(got, dur.cpu().numpy(), t_y.numpy(), t_x.numpy())


def test_global_workspace_shape_is_exact():
    """Ty x ceil(Tx/64) x 8 B = 528 KB per utterance: the decision bits go to the global workspace."""
    from stabletts_amd import _lib
    from stabletts_amd.alignment import maximum_path
    assert _lib.load().st_maximum_path_workspace_bytes(2, 6000, 700) > 0
    t_y, t_x = torch.tensor([6000, 4321]), torch.tensor([700, 555])
    nc, _ = _neg_cent(2, 80, 6000, 700, t_y, t_x, seed=6)
    path, dur = maximum_path(nc, t_y, t_x, durations=True)
    ref = mr.maximum_path(nc.cpu().numpy(), t_y.numpy(), t_x.numpy())
    assert np.array_equal(path.cpu().numpy(), ref.astype(np.float32))
    _check_structure(path.cpu().numpy(), dur.cpu().numpy(), t_y.numpy(), t_x.numpy())


def test_widest_supported_tx_is_exact_and_wider_is_rejected():
    from stabletts_amd._lib import NativeError, ST_ERR_UNSUPPORTED
    from stabletts_amd.alignment import maximum_path
    gen = torch.Generator().manual_seed(7)
    Ty, Tx = 4400, 4096
    t_y, t_x = torch.tensor([4400, 3000]), torch.tensor([4096, 3500])          # the second item has t_x > t_y
    nc = (torch.randn(2, Ty, Tx, generator=gen) * 4).cuda()
    path, dur = maximum_path(nc, t_y, t_x, durations=True)
    ref = mr.maximum_path(nc.cpu().numpy(), t_y.numpy(), t_x.numpy())
    assert np.array_equal(path.cpu().numpy(), ref.astype(np.float32))
    _check_structure(path.cpu().numpy(), dur.cpu().numpy(), t_y.numpy(), t_x.numpy())
    with pytest.raises(NativeError) as e:
        maximum_path(torch.zeros(1, 8, Tx + 1, device="cuda"), torch.tensor([8]), torch.tensor([Tx + 1]))
    assert e.value.code == ST_ERR_UNSUPPORTED and "4096" in str(e.value)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_precision_input_keeps_its_dtype(gold, dtype):
    from stabletts_amd.monotonic_align import maximum_path
    nc = torch.from_numpy(gold["ragged/neg_cent"]).to(dtype).cuda()
    mask = torch.from_numpy(gold["ragged/mask"]).cuda()
    path = maximum_path(nc, mask)
    assert path.dtype == dtype and path.device == nc.device
    t_y, t_x = mr.lengths_from_mask(gold["ragged/mask"])
    ref = mr.maximum_path(nc.float().cpu().numpy(), t_y, t_x)                   # the reference's astype(float32)
    assert np.array_equal(path.float().cpu().numpy(), ref.astype(np.float32))


def test_non_contiguous_input_is_read_and_left_unchanged(gold):
    from stabletts_amd.monotonic_align import maximum_path
    base = torch.from_numpy(gold["ties/neg_cent"]).cuda()
    view = base.transpose(1, 2).contiguous().transpose(1, 2)                    # same values, (B, Ty, Tx) strides of a transpose
    assert not view.is_contiguous()
    before = view.clone()
    path = maximum_path(view, torch.from_numpy(gold["ties/mask"]).cuda())
    assert torch.equal(path.cpu(), torch.from_numpy(gold["ties/path"]))
    assert torch.equal(view, before)
    nc = torch.from_numpy(gold["ragged/neg_cent"]).cuda()
    before = nc.clone()
    maximum_path(nc, torch.from_numpy(gold["ragged/mask"]).cuda())
    assert torch.equal(nc, before)                                              # fp32 contiguous: used in place, never written


def test_empty_items_give_zero_paths():
    """t_x == 0 or t_y == 0: an all-zero path and zero durations (the reference's negative-index write is not reproduced)."""
    from stabletts_amd.alignment import maximum_path
    t_y, t_x = torch.tensor([50, 0, 40, 37]), torch.tensor([0, 12, 20, 15])
    nc, _ = _neg_cent(4, 16, 50, 20, t_y, t_x, seed=8)
    path, dur = maximum_path(nc, t_y, t_x, durations=True)
    assert (path[:2] == 0).all() and (dur[:2] == 0).all()
    ref = mr.maximum_path(nc.cpu().numpy(), t_y.numpy(), t_x.numpy())
    assert np.array_equal(path.cpu().numpy(), ref.astype(np.float32))
    assert torch.equal(dur[2:].cpu(), path[2:].sum(1).to(torch.int32).cpu())


@pytest.mark.parametrize("B,D,Tx,Ty", [(4, 80, 300, 900), (3, 100, 77, 130), (2, 7, 1, 65)])
def test_fused_neg_cent_against_fp64(B, D, Tx, Ty):
    from stabletts_amd.alignment import mas_neg_cent
    gen = torch.Generator().manual_seed(B * 1000 + D)
    mu_x = torch.randn(B, D, Tx, generator=gen)
    y = torch.randn(B, D, Ty, generator=gen) * 1.5
    got = mas_neg_cent(mu_x.cuda(), y.cuda()).cpu().double()
    m, yy = mu_x.double(), y.double()
    ref = (D * (-0.5 * math.log(2 * math.pi)) - 0.5 * (yy ** 2).sum(1)[:, :, None] + torch.einsum("bdt,bds->bts", yy, m)
           - 0.5 * (m ** 2).sum(1)[:, None, :])
    err = float((got - ref).abs().max() / ref.abs().max())
    assert got.shape == (B, Ty, Tx) and err <= 1e-5, err


def test_monotonic_alignment_on_clear_fixture(gold):
    from stabletts_amd.alignment import monotonic_alignment
    g = {k[len("clear/"):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("clear/")}
    mu_x, y, x_mask, y_mask = (g[k].cuda() for k in ("mu_x", "y", "x_mask", "y_mask"))
    out = monotonic_alignment(mu_x, x_mask, y, y_mask)
    attn = out["attn"]
    assert attn.shape == g["attn"].shape and torch.equal(attn.cpu(), g["attn"])
    assert torch.equal(out["durations"].cpu(), g["attn"].sum(2))

    def rel(a, b):
        return float((a.cpu() - b).abs().max() / b.abs().max())

    assert rel(out["logw_"], g["logw_"]) <= 1e-6
    a = attn.squeeze(1).transpose(1, 2)                                         # the caller's matmul, models/model.py:165-167
    mu_y = torch.matmul(a.squeeze(1).transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)
    assert rel(mu_y, g["mu_y"]) <= 1e-6
    D = mu_x.shape[1]
    prior = torch.sum(0.5 * ((y - mu_y) ** 2 + math.log(2 * math.pi)) * y_mask) / (torch.sum(y_mask) * D)
    assert abs(float(prior) - float(g["prior_loss"])) <= 1e-6 * abs(float(g["prior_loss"]))
