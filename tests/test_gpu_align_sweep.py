"""The kernels behind the alignment search at training-size widths, against the float64 restatement
(tests/align_loss_restatement.py) and the length-regulation restatement (tests/align_restatement.py) on the cases of
tests/align_sweep_cases.py: segment_ends at more than one token per thread (Tx > 256, up to the 4096 limit), the backward's
token blocks past the first, a last channel block with fewer channels than waves, tokens that span frame blocks, tokens without
frames on a chunk edge, malformed counts in a chunk's second token, the duration loss past the grid caps of its forward and its
backward, the search chained into the losses, and durations_kernel / align_kernel / path_kernel past 256 tokens.
Gates: those of tests/test_gpu_align_losses.py and tests/test_gpu_alignment.py, through their own functions.  Run with ``-m gpu``.

Measured on an MI355X (profiles/align_sweep_parity.txt): see MEASURED below.
"""
import numpy as np
import pytest
import torch

from oracle.make_golden_align import align_inputs
from tests import align_restatement as lr
from tests import align_sweep_cases as sc
from tests import test_gpu_align_losses as tal

pytestmark = [pytest.mark.gpu, pytest.mark.grad]
U = tal.U

# MEASURED (MI355X, profiles/align_sweep_parity.txt; gates 1e-6, 1, 2.38e-07):
#   shape (B x M x Tx x Ty)   prior_loss rel.   dur_loss rel.   grad_mu_x error / bound   grad_logw rel.
#   2 x 17 x 64 x 255         2.09e-08          7.13e-09        0.199                     5.54e-08
#   2 x 16 x 65 x 256         2.98e-10          4.97e-08        0.197                     5.00e-08
#   2 x 80 x 256 x 257        3.57e-08          5.39e-08        0.200                     5.37e-08
#   2 x 19 x 257 x 513        2.98e-08          1.84e-08        0.200                     5.69e-08
#   3 x 100 x 350 x 1000      1.99e-10          4.87e-08        0.200                     5.60e-08     (the prior loss the fp32 partials
#   1 x 16 x 4096 x 4200      3.24e-08          1.14e-08        0.200                     5.59e-08      were in doubt for)
#   duration grid 17 x 4096   3.93e-08          4.26e-09        0.171                     5.94e-08
#   duration grid 65 x 4096   1.72e-09          1.44e-08        0.178                     5.95e-08
# (0.2 is a one-frame token: half an ulp of the fp32 result against its (1 + 4) 2^-24 S bound.)  A scratch build with a scan that is
# wrong from two tokens per thread on and one-trip duration-loss loops passed every earlier test and failed seven tests here.


def check_against_restatement(label, g, res, f, r):
    """The gates of tests/test_gpu_align_losses.py on one run: outputs equal, losses 1e-6, gradients under their bounds."""
    Tx = g["mu_x"].shape[2]
    assert res["frame_token"].dtype == np.int32 and np.array_equal(res["frame_token"], f["frame_token"])
    assert res["frame_token"].max() < Tx and res["frame_token"].min() >= -1
    assert res["mu_y"].dtype == np.float32 and np.array_equal(res["mu_y"], f["mu_y"].astype(np.float32))
    assert np.array_equal(res["mu_y_masked"], f["mu_y_masked"].astype(np.float32))
    assert np.abs(res["logw_"] - f["logw_"]).max() <= U * np.abs(f["logw_"]).max()
    for k in ("prior_loss", "dur_loss"):
        got, want = float(res[k]), float(f[k])
        print(f"align_sweep {label} {k}: native {got!r}, float64 {want!r}, relative error {abs(got - want) / abs(want):.3g} (gate 1e-06)")
        assert abs(got - want) <= 1e-6 * abs(want)
    print(f"align_sweep {label} gradients:")
    tal.check_grads(res, g, r, r["grad_mu_x"], r["grad_logw"], r["grad_fake_content"])


@pytest.mark.parametrize("shape", list(sc.SCAN_CASES), ids=sc.scan_id)
def test_scan_chunks_against_float64(shape):
    g = sc.scan_case(shape)
    assert sc.zero_token_on_a_chunk_edge(g)
    f, r = sc.restated(("scan", shape))
    print(f"align_sweep {sc.scan_id(shape)}: {sc.scan_chunk(shape[2])} tokens per thread, token blocks {(shape[2] + 63) // 64}, "
          f"channels in the last block {(shape[1] - 1) % 16 + 1}, longest token {int(r['n'].max())} frames, "
          f"tokens without frames {int(((r['n'] == 0) & (g['x_mask'][:, 0] != 0)).sum())}")
    res = tal.run(g)
    check_against_restatement(sc.scan_id(shape), g, res, f, r)
    again = tal.run(g)
    for k in ("frame_token", "mu_y", "mu_y_masked", "prior_loss", "dur_loss", "logw_", "grad_mu_x", "grad_logw", "grad_fake_content"):
        assert np.array_equal(res[k], again[k]), k


@pytest.mark.parametrize("B,Tx", sc.DUR_GRID_SHAPES)
def test_duration_loss_past_its_grid_caps(B, Tx):
    """B Tx > 256 x 256 starts the stride loop of the partial kernel, > 1024 x 256 the backward's: every element of logw_ and of
    grad_logw is compared (the truth of grad_logw is non-zero everywhere, and the output buffers are likely to come back holding
    the NaN written here)."""
    g = sc.duration_grid_case(B, Tx)
    f, r = sc.restated(("grid", (B, Tx)))
    assert (r["grad_logw"] != 0).all()
    stale = [torch.full((B, 1, Tx), float("nan"), device="cuda") for _ in range(4)]
    del stale
    res = tal.run(g)
    assert res["logw_"].shape == (B, 1, Tx) and res["grad_logw"].shape == (B, 1, Tx)
    assert np.isfinite(res["logw_"]).all() and np.isfinite(res["grad_logw"]).all()
    err = np.abs(res["logw_"].astype(np.float64) - f["logw_"])
    assert (err <= U * np.abs(f["logw_"])).all()                                  # element by element, 0 exactly where the truth is 0
    err = np.abs(res["grad_logw"].astype(np.float64) - r["grad_logw"])
    assert (err <= 4 * U * np.abs(r["grad_logw"])).all() and (res["grad_logw"] != 0).all()
    check_against_restatement(f"duration grid {B}x{Tx}", g, res, f, r)


def test_malformed_durations_at_two_tokens_per_thread():
    """tests/test_gpu_align_losses.py::test_malformed_durations_are_clipped where a thread of the scan owns two tokens: the outputs
    are those of the clipped counts as the restatement defines them, and item 0's overflow does not move item 1."""
    g = sc.scan_case(sc.MALFORMED_SHAPE)
    both, only1 = sc.malformed_durations(g)
    f, r = sc.restated(("scan", sc.MALFORMED_SHAPE), "malformed")
    res, base = tal.run(g, durations=both), tal.run(g, durations=only1)
    check_against_restatement("malformed", g, res, f, r)
    clean = sc.restated(("scan", sc.MALFORMED_SHAPE))[0]
    assert not np.array_equal(f["frame_token"][0], clean["frame_token"][0]) and not np.array_equal(f["frame_token"][1], clean["frame_token"][1])
    for k in ("frame_token", "mu_y", "mu_y_masked", "grad_mu_x"):
        assert np.array_equal(res[k][1], base[k][1]), k
    f1, r1 = sc.restated(("scan", sc.MALFORMED_SHAPE), "malformed1")
    check_against_restatement("malformed, item 1 only", g, base, f1, r1)


def test_width_past_the_limit_is_refused_on_the_host():
    from stabletts_amd._lib import NativeError, ST_ERR_UNSUPPORTED
    from stabletts_amd.alignment import align_and_losses
    Tx = 4097
    z = lambda *s: torch.zeros(*s, device="cuda")                                 # noqa: E731
    with pytest.raises(NativeError) as e:
        align_and_losses(z(1, 1, Tx), z(1, 1, Tx) + 1, z(1, 1, Tx), torch.tensor([Tx]).cuda(), z(1, 1, 8), z(1, 1, 8) + 1,
                         torch.zeros(1, Tx, dtype=torch.int32, device="cuda"))
    assert e.value.code == ST_ERR_UNSUPPORTED and "4096" in str(e.value)


def test_search_chained_into_the_losses():
    """monotonic_alignment -> align_and_losses -> dense_alignment at B = 3, M = 80, Tx = 300, Ty = 700: the frame_token the losses
    are computed from is the search's own path, and the dense alignment built from it is that path."""
    from stabletts_amd.alignment import align_and_losses, dense_alignment, monotonic_alignment
    g = sc.case_by_key(("chain",))
    B, M, Tx = g["mu_x"].shape
    t = {k: torch.tensor(g[k]).cuda() for k in ("mu_x", "x_mask", "y", "y_mask", "logw")}
    out = monotonic_alignment(t["mu_x"], t["x_mask"], t["y"], t["y_mask"])
    path = out["attn"][:, 0]                                                      # (B, Ty, Tx)
    assert path.shape == (B, 700, Tx) and torch.equal(out["durations"][:, 0], path.sum(1))
    assert torch.equal(path.sum((1, 2)).cpu(), torch.tensor(g["y_lengths"]).float())
    res = align_and_losses(t["mu_x"], t["x_mask"], t["logw"], torch.tensor(g["x_lengths"]).cuda(), t["y"], t["y_mask"], out["durations"])
    want = torch.where(path.sum(2) > 0, path.argmax(2), -1).to(torch.int32)
    assert torch.equal(res["frame_token"], want)
    assert torch.equal(dense_alignment(res["frame_token"], Tx), path.transpose(1, 2))
    print(f"align_sweep chain: frame_token equals the path's arg-max on {int((want >= 0).sum())} covered frames, "
          f"-1 on {int((want < 0).sum())}")


@pytest.mark.parametrize("name", list(sc.REGULATE_CASES))
def test_length_regulation_past_256_tokens(name):
    """The assertions of tests/test_gpu_alignment.py::test_length_regulate_bit_exact and ::test_generate_path_drop_in_bit_exact
    against the restatement: the second trip of durations_kernel's 256-thread stride, Tx = 256 / 257 / 700."""
    from stabletts_amd.alignment import generate_path, length_regulate
    B, Tx, xl, M, ls, seed = sc.REGULATE_CASES[name]
    logw, mu_x, x_mask, _ = align_inputs(B, Tx, xl, M, seed)
    want = lr.length_regulate(logw, x_mask, mu_x, ls)
    r = length_regulate(logw.cuda(), x_mask.cuda(), mu_x.cuda(), ls)
    assert np.array_equal(r["w_ceil"].cpu().numpy(), want["w_ceil"].numpy())
    assert np.array_equal(r["y_lengths"].cpu().numpy(), want["y_lengths"].numpy())
    assert np.array_equal(r["y_mask"].cpu().numpy(), want["y_mask"].numpy())
    assert np.array_equal(r["attn"][:, 0].cpu().numpy(), want["attn"].numpy())
    assert np.array_equal(r["mu_y"].cpu().numpy(), want["mu_y"].numpy())          # a gather of fp32 values: exact
    r2 = length_regulate(logw.cuda(), x_mask.cuda(), mu_x.cuda(), ls, return_attn=False)
    assert r2["attn"] is None and torch.equal(r2["mu_y"], r["mu_y"])
    attn_mask = x_mask[:, 0, :, None] * want["y_mask"][:, 0, None, :]
    path = generate_path(want["w_ceil"][:, 0].cuda(), attn_mask.cuda())
    assert path.dtype == attn_mask.dtype and np.array_equal(path.cpu().numpy(), want["attn"].numpy())
    print(f"align_sweep regulate {name}: Tx {Tx}, y_lengths {want['y_lengths'].tolist()}, length_scale {ls}: bit-exact")
