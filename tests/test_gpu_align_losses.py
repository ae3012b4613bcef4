"""The training side of the alignment step on a real MI355X (st_align_train_forward / _backward, st_duration_loss /
_backward behind stabletts_amd.alignment.align_and_losses, and stabletts_amd.model.StableTTS on top) against the REAL reference
StableTTS.forward (tests/golden/align_loss_grads.npz, tools/make_golden_align_losses.py) and the float64 restatement
(tests/align_loss_restatement.py).  Run with ``-m gpu``.

Gates.  mu_y, mu_y_masked, frame_token: equal to the reference (a product with a 0/1 matrix is exact in fp32).  Losses: 1e-6
relative to float64 (the bar tests/test_gpu_mas.py uses for the same prior_loss).  grad_mu_x, per element:
|native - f64| <= (n + 4) 2^-24 S, n the frames of the token and S the float64 sum of |term| over the element's sum: the bound of
a sequential fp32 sum of n terms that each carry a few roundings (the kernels accumulate in fp64, so they sit far inside it);
exactly 0 for a token without frames.  grad_fake_content: the same bound with n = the terms one thread sums plus the 8 adds of
the tree.  grad_logw: 4 x 2^-24 relative per element.  Parameter gradients of the whole model: see the end-to-end test.
"""
import math

import numpy as np
import pytest
import torch

from tests import align_loss_restatement as ar
from tests.align_loss_restatement import CASES, GOLDEN, case_of

pytestmark = [pytest.mark.gpu, pytest.mark.grad]
U = 2.0 ** -24
INPUTS = ("mu_x", "logw", "y", "W", "fake_content", "x_mask", "y_mask")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def run(g, durations=None, keep="case", prior=True, dur=True, extra=None, items=None):
    """align_and_losses on a fixture case (or on `items` of it alone) and the gradients of
    [dur_loss] + [prior_loss] + sum(W * mu_y_masked) [+ sum(extra * mu_y)].  -> dict of numpy arrays."""
    from stabletts_amd.alignment import align_and_losses
    sl = slice(None) if items is None else items
    t = {k: torch.from_numpy(g[k][sl] if k != "fake_content" else g[k]).cuda() for k in INPUTS}
    mu_x, logw, fc = (t[k].clone().requires_grad_(True) for k in ("mu_x", "logw", "fake_content"))
    d = torch.from_numpy((g["durations"] if durations is None else durations)[sl]).cuda()
    kp = torch.from_numpy(g["keep"][sl]).cuda() if isinstance(keep, str) else keep
    out = align_and_losses(mu_x, t["x_mask"], logw, torch.from_numpy(g["x_lengths"][sl]).cuda(), t["y"], t["y_mask"], d, keep=kp,
                           fake_content=fc)
    loss = (t["W"] * out["mu_y_masked"]).sum()
    if prior:
        loss = loss + out["prior_loss"]
    if dur:
        loss = loss + out["dur_loss"]
    if extra is not None:
        loss = loss + (torch.from_numpy(extra[sl]).cuda() * out["mu_y"]).sum()
    grads = torch.autograd.grad(loss, (mu_x, logw, fc), allow_unused=True)
    res = {k: v.detach().cpu().numpy() for k, v in out.items()}
    for k, v in zip(("grad_mu_x", "grad_logw", "grad_fake_content"), grads):
        res[k] = None if v is None else v.cpu().numpy()
    res["out"] = out
    return res


def check_grad_mu_x(got, want, r):
    n = np.broadcast_to(r["n"][:, None, :], want.shape)
    err = np.abs(got.astype(np.float64) - want)
    bound = (n + 4) * U * r["S"]
    worst = float(np.max(err / np.maximum(bound, 1e-300) * (bound > 0)))
    print(f"grad_mu_x: worst error / bound {worst:.3g}, longest segment {int(n.max())}")
    assert (err <= bound).all(), worst
    assert not got.transpose(0, 2, 1)[r["n"] == 0].any()                          # a token without frames: exactly 0


def check_grads(res, g, r, want_mu_x, want_logw, want_fake):
    check_grad_mu_x(res["grad_mu_x"], want_mu_x, r)
    err = np.abs(res["grad_logw"].astype(np.float64) - want_logw)
    print(f"grad_logw: worst relative error {float(np.max(err / np.maximum(np.abs(want_logw), 1e-300) * (want_logw != 0))):.3g} (gate {4 * U:.3g})")
    assert (err <= 4 * U * np.abs(want_logw)).all()
    gf = res["grad_fake_content"].reshape(-1).astype(np.float64)
    assert (np.abs(gf - want_fake.reshape(-1)) <= (r["n_fake"][0] + 8 + 4) * U * r["S_fake"]).all()


def restated_backward(g, durations=None, prior=True, extra=None):
    return ar.backward(g["mu_x64"], g["x_mask"], g["logw64"], g["x_lengths"], g["y64"], g["y_mask"],
                       g["durations"] if durations is None else durations, g["keep"], g_masked=g["W64"],
                       g_mu_y=None if extra is None else extra.astype(np.float64), g_prior=1.0 if prior else None, g_dur=1.0)


@pytest.mark.parametrize("case", CASES)
def test_outputs_equal_the_reference(gold, case):
    g = case_of(gold, case)
    res = run(g)
    attn = g["attn"]
    assert res["frame_token"].dtype == np.int32
    assert np.array_equal(res["frame_token"], np.where(attn.sum(1) == 1, attn.argmax(1), -1))
    assert res["mu_y"].dtype == np.float32 and np.array_equal(res["mu_y"], g["mu_y"])
    assert np.array_equal(res["mu_y_masked"], g["mu_y_masked"])
    if not g["keep"].all():      # a dropped item holds fake_content in every frame, padded frames included
        b = int(np.flatnonzero(~g["keep"])[0])
        assert np.array_equal(res["mu_y_masked"][b], np.broadcast_to(g["fake_content"][0], res["mu_y_masked"][b].shape))
    logw_ = np.log(1e-8 + g["durations"].astype(np.float64))[:, None] * g["x_mask"]
    assert np.abs(res["logw_"] - logw_).max() <= U * np.abs(logw_).max()


@pytest.mark.parametrize("case", CASES)
def test_losses_against_float64(gold, case):
    g = case_of(gold, case)
    res = run(g)
    for k in ("prior_loss", "dur_loss"):
        got, want = float(res[k]), float(g[k + "_f64"].reshape(-1)[0])
        print(f"{case} {k}: native {got!r}, float64 {want!r}, relative error {abs(got - want) / abs(want):.3g}")
        assert abs(got - want) <= 1e-6 * abs(want)


@pytest.mark.parametrize("case", CASES)
def test_gradients_against_float64(gold, case):
    g = case_of(gold, case)
    res = run(g)
    r = restated_backward(g)
    check_grads(res, g, r, g["grad_mu_x_f64"], g["grad_logw_f64"], g["grad_fake_content_f64"])


def test_autograd_wiring(gold):
    g = case_of(gold, "ragged")
    res = run(g)
    out = res["out"]
    for k in ("mu_y", "mu_y_masked", "prior_loss", "dur_loss"):
        assert out[k].grad_fn is not None and out[k].requires_grad, k
    assert not out["logw_"].requires_grad and not out["frame_token"].requires_grad
    assert out["prior_loss"].shape == () and out["dur_loss"].shape == () and out["logw_"].shape == g["logw"].shape
    assert res["grad_fake_content"].shape == g["fake_content"].shape
    from stabletts_amd.alignment import align_and_losses
    t = {k: torch.from_numpy(g[k]).cuda() for k in INPUTS}
    mu_x, logw = t["mu_x"].clone().requires_grad_(True), t["logw"].clone().requires_grad_(True)
    o = align_and_losses(mu_x, t["x_mask"], logw, torch.from_numpy(g["x_lengths"]).cuda(), t["y"], t["y_mask"],
                         torch.from_numpy(g["durations"]).cuda())
    gm, gl = torch.autograd.grad(o["dur_loss"], (mu_x, logw), allow_unused=True)
    assert gm is None and gl is not None
    assert torch.equal(o["mu_y"], o["mu_y_masked"])                                # no keep, no fake_content: nothing masked


def test_two_runs_are_bitwise_equal(gold):
    g = case_of(gold, "ragged")
    a, b = run(g, extra=g["W"][:, ::-1].copy()), run(g, extra=g["W"][:, ::-1].copy())
    for k in ("frame_token", "mu_y", "mu_y_masked", "prior_loss", "dur_loss", "logw_", "grad_mu_x", "grad_logw", "grad_fake_content"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("case", ["ragged", "wide"])
def test_an_item_alone_equals_the_item_in_the_batch(gold, case):
    g = case_of(gold, case)
    extra = g["W"][:, ::-1].copy()
    whole = run(g, prior=False, extra=extra)
    for b in range(g["mu_x"].shape[0]):
        alone = run(g, prior=False, extra=extra, items=slice(b, b + 1))
        for k in ("frame_token", "mu_y", "mu_y_masked", "grad_mu_x"):
            assert np.array_equal(alone[k][0], whole[k][b]), (k, b)


def test_malformed_durations_are_clipped(gold):
    """Item 1's counts sum past Ty, item 2 holds a negative count, item 3 a count behind its x_mask.  Every buffer is of the
    size the kernels are told, and every index is clipped before use: the outputs are those of the clipped counts, as the
    restatement defines them, and the neighbours do not move."""
    g = case_of(gold, "ragged")
    Ty = g["y"].shape[2]
    dur = g["durations"].copy()
    dur[1, 3] += 50
    dur[2, 5] = -4
    dur[3, 20] = 7
    assert dur[1].sum() > Ty and g["x_mask"][3, 0, 20] == 0
    ends = ar.segment_ends(dur, g["x_mask"], Ty)
    assert ends.max() == Ty and ends[2, 5] == ends[2, 4] and ends[3, 20] == ends[3, 19]
    res, base = run(g, durations=dur), run(g)
    f = ar.forward(g["mu_x64"], g["x_mask"], g["logw64"], g["x_lengths"], g["y64"], g["y_mask"], dur, g["keep"], g["fake_content64"])
    assert np.array_equal(res["frame_token"], f["frame_token"]) and res["frame_token"].max() < g["mu_x"].shape[2]
    assert np.array_equal(res["mu_y"], f["mu_y"].astype(np.float32))
    assert np.array_equal(res["mu_y_masked"], f["mu_y_masked"].astype(np.float32))
    assert abs(float(res["prior_loss"]) - f["prior_loss"]) <= 1e-6 * f["prior_loss"]
    assert abs(float(res["dur_loss"]) - f["dur_loss"]) <= 1e-6 * f["dur_loss"]
    r = restated_backward(g, durations=dur)
    check_grads(res, g, r, r["grad_mu_x"], r["grad_logw"], r["grad_fake_content"])
    for b in (0, 3):                       # (item 3's stray count sits behind its mask: it changes nothing)
        for k in ("frame_token", "mu_y", "mu_y_masked", "grad_mu_x"):
            assert np.array_equal(res[k][b], base[k][b]), (k, b)
    assert np.array_equal(res["grad_logw"][0], base["grad_logw"][0])


# ---- the whole model: stabletts_amd.model.StableTTS against the reference's glue lines written in torch around the same submodules
def small_model():
    import oracle
    from oracle.weights import DecoderConfig, TextEncoderConfig
    from stabletts_amd.model import StableTTS
    torch.manual_seed(11)
    # (the estimator pairs its layers through long skip connections: 2 is its smallest depth)
    model = StableTTS(401, 128, 256, 1024, 4, 1, 2, 3, 0.1, 256)
    model.encoder.load_state_dict(oracle.make_text_encoder_state_dict(2468, TextEncoderConfig(n_layers=1), ada_std=0.15))
    model.decoder.estimator.load_state_dict(oracle.make_state_dict(1234, DecoderConfig(n_layers=2), ada_std=0.15))
    with torch.no_grad():
        model.fake_content.normal_(0, 0.5)
        model.fake_speaker.normal_(0, 0.5)
    return model.cuda().eval()


def batch():
    gen = torch.Generator().manual_seed(7)
    B, Tx, Ty = 3, 24, 96
    x = torch.randint(1, 401, (B, Tx), generator=gen).cuda()
    y = torch.randn(B, 128, Ty, generator=gen).cuda()
    return (x, torch.tensor([24, 17, 9]).cuda(), y, torch.tensor([96, 70, 41]).cuda(), y[:, :, :48].contiguous(),
            torch.tensor([48, 40, 30]).cuda())


def glue_run(model, data, seed, dtype):
    """models/model.py:136-178 in torch around the model's own submodules, the lines behind the alignment search in `dtype`.
    mu_y is a gather by the search's own path, so no GEMM precision enters; the decoder gets fp32, exactly."""
    from stabletts_amd.alignment import monotonic_alignment
    from stabletts_amd.model import sequence_mask
    x, x_lengths, y, y_lengths, z, z_lengths = data
    B, M, Ty = y.shape
    torch.manual_seed(seed)
    y_mask = sequence_mask(y_lengths, y.size(2)).unsqueeze(1).to(y.dtype)
    z_mask = sequence_mask(z_lengths, z.size(2)).unsqueeze(1).to(z.dtype)
    cfg_mask = torch.rand(y.size(0), 1, device=y.device) > model.cfg_dropout
    c = model.ref_encoder(z, z_mask) * cfg_mask + ~cfg_mask * model.fake_speaker.repeat(z.size(0), 1)
    h, mu_x, x_mask = model.encoder(x, c, x_lengths)
    logw = model.dp(h, x_mask, c)
    attn = monotonic_alignment(mu_x, x_mask, y, y_mask)["attn"]
    mu_x_d = mu_x.to(dtype)
    mu_x_d.retain_grad()
    logw_ = torch.log(1e-8 + attn.sum(2).to(dtype)) * x_mask.to(dtype)
    dur_loss = torch.sum((logw.to(dtype) - logw_) ** 2) / torch.sum(x_lengths)
    path = attn.squeeze(1)                                                       # (B, Ty, Tx)
    covered, tok = path.sum(2) > 0, path.argmax(2)
    mu_y = torch.gather(mu_x_d, 2, tok[:, None, :].expand(B, M, Ty)) * covered[:, None, :].to(dtype)
    cm = cfg_mask.unsqueeze(-1)
    mu_y_masked = mu_y * cm + ~cm * model.fake_content.to(dtype).repeat(mu_y.size(0), 1, mu_y.size(-1))
    mu_y_masked.retain_grad()
    diff_loss, _ = model.decoder.compute_loss(y, y_mask, mu_y_masked.float(), c)
    prior_loss = torch.sum(0.5 * ((y.to(dtype) - mu_y) ** 2 + math.log(2 * math.pi)) * y_mask.to(dtype))
    prior_loss = prior_loss / (torch.sum(y_mask.to(dtype)) * M)
    model.zero_grad(set_to_none=True)
    (dur_loss + diff_loss + prior_loss).backward()
    return dict(dur_loss=dur_loss.detach(), diff_loss=diff_loss.detach(), prior_loss=prior_loss.detach(), cfg_mask=cfg_mask,
                mu_x=mu_x.detach(), grad_mu_x=mu_x_d.grad, g_masked=mu_y_masked.grad, attn=path.transpose(1, 2), x_mask=x_mask.detach(),
                y_mask=y_mask, durations=attn.sum(2)[:, 0].to(torch.int32), logw=logw.detach(),
                grads={n: p.grad.detach().clone() for n, p in model.named_parameters()})


def test_model_forward_and_backward_against_the_torch_glue():
    """Run A: the native StableTTS.  Run B: the same submodules with the glue in torch, once in fp32 and once in float64.
    Losses as above; diff_loss bitwise (the decoder sees identical inputs); mu_x.grad under the segmented-sum bound; parameter
    gradients per tensor relative to the tensor's max-abs: with A = |native - glue64| and B = |glue32 - glue64|, A <= 4 B + 1e-7
    (both are fp32 roundings of one quantity in different orders)."""
    model, data = small_model(), batch()
    seed = next(s for s in range(50) if 0 < int((torch.manual_seed(s) and torch.rand(3, 1, device="cuda") > 0.2).sum()) < 3)
    seen = {}

    def keep_mu_x(_module, _inputs, output):
        output[1].retain_grad()
        seen["mu_x"] = output[1]

    hook = model.encoder.register_forward_hook(keep_mu_x)
    torch.manual_seed(seed)
    model.zero_grad(set_to_none=True)
    dur_loss, diff_loss, prior_loss, attn = model(*data)
    (dur_loss + diff_loss + prior_loss).backward()
    hook.remove()
    native = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    assert all(v is not None for v in native.values())
    g32, g64 = glue_run(model, data, seed, torch.float32), glue_run(model, data, seed, torch.float64)
    assert g64["cfg_mask"].any() and not g64["cfg_mask"].all()
    assert torch.equal(attn, g64["attn"]) and attn.shape == (3, 24, 96) and torch.equal(seen["mu_x"].detach(), g64["mu_x"])
    for k, got in (("prior_loss", prior_loss), ("dur_loss", dur_loss)):
        got, want = float(got.detach()), float(g64[k])
        print(f"model {k}: native {got!r}, float64 glue {want!r}")
        assert abs(got - want) <= 1e-6 * abs(want)
    assert torch.equal(diff_loss, g64["diff_loss"]) and torch.equal(diff_loss, g32["diff_loss"])
    r = ar.backward(g64["mu_x"].double().cpu().numpy(), g64["x_mask"].cpu().numpy(), g64["logw"].double().cpu().numpy(),
                    data[1].cpu().numpy(), data[2].double().cpu().numpy(), g64["y_mask"].cpu().numpy(), g64["durations"].cpu().numpy(),
                    g64["cfg_mask"].cpu().numpy(), g_masked=g64["g_masked"].cpu().numpy(), g_prior=1.0, g_dur=1.0)
    assert np.abs(r["grad_mu_x"] - g64["grad_mu_x"].cpu().numpy()).max() <= 1e-12 * np.abs(r["grad_mu_x"]).max()
    check_grad_mu_x(seen["mu_x"].grad.cpu().numpy(), g64["grad_mu_x"].cpu().numpy(), r)
    lines, bad = [], {}
    for module in ("encoder", "ref_encoder", "dp", "decoder", "fake_speaker", "fake_content"):
        worst = (0.0, 0.0)
        for n in native:
            if n.split(".")[0] != module:
                continue
            ref = g64["grads"][n].double()
            scale = max(float(ref.abs().max()), 1e-30)
            a = float((native[n].double() - ref).abs().max()) / scale
            b = float((g32["grads"][n].double() - ref).abs().max()) / scale
            worst = max(worst, (a, b))
            if a > 4 * b + 1e-7:
                bad[n] = (a, b)
        lines.append(f"align_loss_parity {module:<12} A (native glue vs float64 glue) {worst[0]:.3e}   B (fp32 torch glue vs float64 glue) {worst[1]:.3e}")
    print("\n".join(lines))
    assert not bad, bad


def test_model_synthesise_equals_the_existing_chain():
    from stabletts_amd.alignment import length_regulate
    model, data = small_model(), batch()
    x, x_lengths, y = data[0], data[1], data[2]
    with torch.no_grad():
        torch.manual_seed(5)
        got = model.synthesise(x, x_lengths, 2, temperature=0.8, y=y, length_scale=1.0, solver="euler", cfg=2.0)
        torch.manual_seed(5)
        c = model.ref_encoder(y, None)
        h, mu_x, x_mask = model.encoder(x, c, x_lengths)
        lr = length_regulate(model.dp(h, x_mask, c), x_mask, mu_x, 1.0)
        want = model.decoder(lr["mu_y"], lr["y_mask"], 2, 0.8, c, "euler",
                             {"fake_speaker": model.fake_speaker, "fake_content": model.fake_content, "cfg_strength": 2.0})
    assert set(got) == {"encoder_outputs", "decoder_outputs", "attn"}
    assert torch.equal(got["encoder_outputs"], lr["mu_y"]) and torch.equal(got["attn"], lr["attn"])
    assert torch.equal(got["decoder_outputs"], want) and torch.isfinite(want).all()
    assert got["decoder_outputs"].is_inference()
