"""Pins tests/style_dp_restatement.py (the reference of the dropout, AdamW, chain and configuration tests of the native
MelStyleEncoder / DurationPredictor) to the REAL modules, on the CPU: style_forward / dp_forward in float64 with the seeded
weights and inputs must reproduce the real modules' fixtures

  * tests/golden/synthesise_outputs.npz (c, logw) and tests/golden/style_dp_grads.npz (losses, gradient norms, full or sampled
    gradients) within the gates the GPU tests use on the same fixtures, and
  * tests/golden/style_dp_configs.npz (tools/make_golden_style_dp_configs.py: four more configurations of each module, T at the
    tile edges, masks with holes, the split-K sizes) within HALF of each gate, so that at least half of every gate of
    tests/test_gpu_style_duration_configs.py belongs to the kernels, whichever of the two references they are compared with.

Gates: c max abs error / max |c| <= 1e-5; logw <= 1e-4 absolute on valid tokens and exactly 0 on padded ones; loss <= 1e-5
relative; gradients max |a - b| / max |b| <= 1e-4 per tensor and norms within 1e-4.

ReLU kinks of the DurationPredictor (a condition of the cases, not a tolerance): a pre-activation within rounding of 0 makes
fp32 and float64 take different branches, and the gradient then differs by a whole term.  Cases above
synth_weights.KINK_FREE_ABOVE pre-activations use the kink-free weights: asserted here, every |pre-activation| of a valid token
>= 0.5 (the biases are +-U(1, 2), the conv term 0.1 x a unit-variance input's: a 5 sigma excursion stays below 0.5) with between
30 % and 70 % of them positive, so the backward's ReLU mask is exercised.  The smaller cases keep realistic weights whose seed
was searched: asserted here, min |float64 pre-activation| >= 32 x max |fp32 - float64 pre-activation| (the fp32 restatement is
the same torch calls as the real module), which leaves a native summation order 32 x worse than torch's without a flip.

Measured here (float64 restatement against the real fp32 modules' fixtures): c <= 7.7e-7, logw <= 2.5e-6, style gradients
<= 4.7e-6, predictor gradients <= 2.8e-5, losses <= 2.7e-6."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import style_dp_restatement as R  # noqa: E402
import synth_weights as sw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_GATE, LOGW_GATE, LOSS_GATE, GRAD_GATE = 1e-5, 1e-4, 1e-5, 1e-4
KINK_FACTOR = 32.0


def _gold(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


@pytest.fixture(scope="module")
def synth():
    return _gold("synthesise_outputs.npz")


@pytest.fixture(scope="module")
def grads():
    return _gold("style_dp_grads.npz")


@pytest.fixture(scope="module")
def configs():
    return _gold("style_dp_configs.npz")


def _scalar(a):
    return float(np.asarray(a).reshape(-1)[0])


def _c_err(c, ref):
    assert c.shape == ref.shape
    return float(np.abs(c - ref).max() / np.abs(ref).max())


def _logw_err(lw, ref, mask):
    assert lw.shape == ref.shape
    assert np.all(lw[mask == 0] == 0.0) and np.all(ref[mask == 0] == 0.0)
    return float(np.abs(lw - ref)[mask > 0].max())


def _old_digest(gold, case):
    """style_dp_grads.npz keeps one array per parameter: the same digest, rebuilt."""
    names = gold[f"{case}/names"].tolist()
    part = lambda kind: [gold[f"{case}/{kind}/{n}"] for n in names if f"{case}/{kind}/{n}" in gold.files]      # noqa: E731
    return dict(names=names, norms=gold[f"{case}/norms"], absmax=gold[f"{case}/absmax"], full=np.concatenate(part("full")),
                sample=np.concatenate(part("sample")))


def _check_grads(ref, got, seed, loss, ref_loss, scale, what):
    if scale < 1.0:
        # the loss gate is relative with a floor of 1: a projection that cancels to |loss| < 1 would turn it into an absolute
        # gate on a sum of hundreds of fp32 terms; the input seeds of the new cases were moved on until |loss| >= 1
        assert abs(loss) >= 1.0, (what, loss)
    assert abs(loss - ref_loss) <= scale * LOSS_GATE * max(abs(ref_loss), 1.0), (what, loss, ref_loss)
    errs = R.digest_errors(ref, got, seed)
    worst = max(errs, key=lambda n: errs[n][0])
    print(f"{what}: loss {abs(loss - ref_loss) / max(abs(ref_loss), 1.0):.1e}, worst gradient {errs[worst][0]:.2e} ({worst}), "
          f"worst norm {max(e[1] for e in errs.values()):.2e}")
    bad = {n: e for n, e in errs.items() if e[0] > scale * GRAD_GATE or e[1] > scale * GRAD_GATE}
    assert not bad, (what, bad)


# ---- 1. the fixtures that exist: the gates of the GPU tests
@pytest.mark.parametrize("case", list(sw.STYLE_CASES))
def test_style_forward_reproduces_the_synthesise_fixture(synth, case):
    B, T, lengths, seed = sw.STYLE_CASES[case]
    y, m = sw.style_inputs(B, T, lengths, seed)
    c, _, _ = R.run_style(sw.style_encoder_state_dict(), y, m, seed)
    err = _c_err(c, synth[case + "_c"])
    print(f"{case}: c {err:.2e}")
    assert err <= C_GATE


@pytest.mark.parametrize("case", list(sw.DP_CASES))
def test_dp_forward_reproduces_the_synthesise_fixture(synth, case):
    B, T, lengths, seed = sw.DP_CASES[case]
    x, m, g = sw.dp_inputs(B, T, lengths, seed)
    logw, _, _, _ = R.run_dp(sw.duration_predictor_state_dict(), x, m, g, seed)
    err = _logw_err(logw, synth[case + "_logw"], m)
    print(f"{case}: logw {err:.2e}")
    assert err <= LOGW_GATE


@pytest.mark.parametrize("case", list(R.STYLE_GRAD_CASES))
def test_style_forward_reproduces_the_gradient_fixture(grads, case):
    B, T, lengths, seed = R.STYLE_GRAD_CASES[case]
    y, m = sw.style_inputs(B, T, lengths, seed)
    _, loss, got = R.run_style(sw.style_encoder_state_dict(), y, m, seed)
    _check_grads(_old_digest(grads, case), got, seed, loss, _scalar(grads[f"{case}/loss"]), 1.0, case)


@pytest.mark.parametrize("case", list(R.DP_GRAD_CASES))
def test_dp_forward_reproduces_the_gradient_fixture(grads, case):
    B, T, lengths, seed = R.DP_GRAD_CASES[case]
    x, m, g = sw.dp_inputs(B, T, lengths, seed)
    _, loss, got, _ = R.run_dp(sw.duration_predictor_state_dict(), x, m, g, seed)
    _check_grads(_old_digest(grads, case), got, seed, loss, _scalar(grads[f"{case}/loss"]), 1.0, case)


# ---- 2. the configurations, tile edges, masks and split-K sizes: half of each gate
def _new_digest(gold, case):
    return {k: gold[f"{case}/{k}"] for k in ("names", "norms", "absmax", "full", "sample")}


@pytest.mark.parametrize("case", list(sw.STYLE_ALL_CASES))
def test_style_forward_reproduces_the_config_fixture(configs, case):
    cfg, B, T, spec, seed = sw.STYLE_ALL_CASES[case]
    y, m = sw.style_config_inputs(case)
    c, loss, got = R.run_style(sw.style_config_state_dict(cfg), y, m, seed, n_head=cfg[4])
    err = _c_err(c, configs[f"{case}/out"])
    print(f"{case}: c {err:.2e}")
    assert err <= 0.5 * C_GATE
    _check_grads(_new_digest(configs, case), got, seed, loss, _scalar(configs[f"{case}/loss"]), 0.5, case)


def _kink_check(case, cfg, lengths, pre64, pre32, m):
    lo, diff = R.kink_margin(pre64, pre32, m)
    valid = torch.from_numpy(m != 0).expand_as(pre64[0])
    on = float(np.mean([float((p[valid] > 0).double().mean()) for p in pre64]))
    print(f"{case}: min |pre-activation| {lo:.3e}, fp32 vs float64 {diff:.3e}, active {on:.2f}")
    assert lo >= KINK_FACTOR * diff, (case, lo, diff)
    if sw.dp_kink_free(cfg, lengths):
        assert lo >= 0.5 and 0.3 <= on <= 0.7, (case, lo, on)


@pytest.mark.parametrize("case", list(sw.DP_ALL_CASES))
def test_dp_forward_reproduces_the_config_fixture(configs, case):
    cfg, B, T, lengths, seed, wseed = sw.DP_ALL_CASES[case]
    x, m, g = sw.dp_config_inputs(case)
    sd = sw.dp_config_state_dict(case)
    logw, loss, got, pre64 = R.run_dp(sd, x, m, g, seed)
    with torch.no_grad():
        _, pre32 = R.dp_forward(sd, torch.from_numpy(x), torch.from_numpy(m), torch.from_numpy(g), return_pre=True)
    _kink_check(case, cfg, lengths, pre64, pre32, m)
    err = _logw_err(logw, configs[f"{case}/out"], m)
    print(f"{case}: logw {err:.2e}")
    assert err <= 0.5 * LOGW_GATE
    _check_grads(_new_digest(configs, case), got, seed, loss, _scalar(configs[f"{case}/loss"]), 0.5, case)


def test_dp_dropout_case_keeps_the_kink_margin():
    """The predictor's dropout case of the GPU tests: under the masks of its seed the pre-activations keep the same margin."""
    case, tseed, p = sw.DP_DROPOUT_CASE
    cfg, B, T, lengths, seed, wseed = sw.DP_ALL_CASES[case]
    torch.manual_seed(tseed)
    drops = R.dp_drops(int(torch.randint(0, 2 ** 62, (1,)).item()), p, B, cfg[1], T)
    x, m, g = sw.dp_config_inputs(case)
    sd = sw.dp_config_state_dict(case)
    _, _, _, pre64 = R.run_dp(sd, x, m, g, seed, drop=drops)
    with torch.no_grad():
        _, pre32 = R.dp_forward(sd, torch.from_numpy(x), torch.from_numpy(m), torch.from_numpy(g), drop=drops, return_pre=True)
    _kink_check(case + " (dropout)", cfg, lengths, pre64, pre32, m)


# ---- 3. the tables themselves
def test_case_tables_cover_what_they_claim():
    edge_t = {1, 2, 63, 64, 65, 128, 129, 257}
    for cases, configs_ in ((sw.STYLE_CONFIG_CASES, sw.STYLE_CONFIGS), (sw.DP_CONFIG_CASES, sw.DP_CONFIGS)):
        assert {v[2] for v in cases.values()} == edge_t
        for cfg in configs_.values():
            ts = sorted(v[2] for v in cases.values() if v[0] == cfg)
            # below a 64-frame tile edge, at one, one frame above one
            assert any(t < 64 for t in ts) and any(t % 64 == 0 for t in ts) and any(t > 64 and t % 64 == 1 for t in ts), (cfg, ts)
        assert all(v[1] > 1 and (v[2] == 1 or len(set(v[3])) > 1) for v in cases.values())      # B > 1, ragged
    for cfg, B, T, spec, seed in sw.STYLE_MASK_CASES.values():
        m = sw.mask_from_spec(B, T, spec)[:, 0]
        assert T >= 129 and not m[0, :70].any() and m[0, 70:].all()          # frames 0..69 invalid
        assert any(m[b].sum() == 1 for b in range(B))                        # a single valid frame
        holes = [b for b in range(B) if m[b].sum() > 1 and np.abs(np.diff(m[b])).sum() > 2]
        assert holes                                                         # interior holes
    assert all(cfg[1] == 64 * cfg[4] and cfg[3] in (1, 3, 5) for cfg in sw.STYLE_CONFIGS.values())
    assert all(cfg[1] % 128 == 0 and cfg[2] in (1, 3, 5) for cfg in sw.DP_CONFIGS.values())
    size = lambda f: os.path.getsize(os.path.join(ROOT, "tests", "golden", f))      # noqa: E731
    assert size("style_dp_configs.npz") <= size("reference_outputs.npz")
