"""Native MelStyleEncoder / DurationPredictor across their configurations, at the tile edges, under masks no prefix gives, and
through every shape of the split-K weight gradient, on a real MI355X.  Run with ``-m gpu`` (``-s`` prints the worst value per case).

Every case (tests/synth_weights.py: STYLE_ALL_CASES, DP_ALL_CASES) is compared twice: with the REAL reference modules' fp32
output, loss and gradients (tests/golden/style_dp_configs.npz, tools/make_golden_style_dp_configs.py) and with the float64
restatement (tests/style_dp_restatement.py, which tests/test_style_dp_restatement_cpu.py pins to the real modules within half of
each gate).  Gates, the project's: c max abs error / max |c| <= 1e-5; logw <= 1e-4 absolute on valid tokens, exactly 0 on padded
ones; loss <= 1e-5 relative; gradients max |native - ref| / max |ref| <= 1e-4 per tensor and the norm within 1e-4.

What the cases reach that the default point (style 128/128/256/k5/2 heads, predictor 256/1024/k3/256) does not: the ci < Cin tail
of sd_conv_kernel's 16-channel chunk (Cin 100, 17, 24), partial 64-channel output tiles (Cout 100, 65), 1, 3 and 5 taps on both
modules' convs in the forward and the tap-flipped data gradient, 1, 3 and 4 attention heads, T on both sides of the 64-frame
tiles, key tiles that are masked before the first valid key, holes and a single valid frame, LayerNorm / GLU / mean-pool /
dropout layouts 64 to 768 channels wide, and wgrad_split's shapes (test_split_k_shapes_are_all_covered lists them).

ReLU kinks: the predictor cases either use kink-free weights or a weight seed whose pre-activations keep 32 x the fp32 rounding
error away from 0 (asserted on the CPU, test_style_dp_restatement_cpu.py), so a difference here is the kernels', not a flipped ReLU.

The two references against each other (real fp32 modules vs float64, measured on the CPU, worst over these cases): c 7.7e-7,
logw 2.1e-6, losses 2.7e-6, style gradients 4.5e-6, predictor gradients 1.2e-5 (a near-zero norm2.bias).
NOT YET MEASURED on an MI355X: this file has not had a GPU run (none was available when it was written), so there are no native
worst values to quote here and no profiles/style_dp_config_sweep.txt yet; the first ``-m gpu -s`` run should add both.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import style_dp_restatement as R  # noqa: E402
import synth_weights as sw  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.grad]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_GATE, LOGW_GATE, LOSS_GATE, GRAD_GATE = 1e-5, 1e-4, 1e-5, 1e-4
_REF64 = {}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "style_dp_configs.npz"))


def _scalar(a):
    return float(np.asarray(a).reshape(-1)[0])


def _style(cfg, train, dropout=0.25):
    if train:
        from stabletts_amd.reference_encoder_train import MelStyleEncoder
    else:
        from stabletts_amd.reference_encoder import MelStyleEncoder
    m = MelStyleEncoder(cfg[0], style_hidden=cfg[1], style_vector_dim=cfg[2], style_kernel_size=cfg[3], style_head=cfg[4], dropout=dropout)
    m.load_state_dict(sw.style_config_state_dict(cfg), strict=True)
    return m.cuda()


def _dp(case, train, p=0.5):
    if train:
        from stabletts_amd.duration_predictor_train import DurationPredictor
    else:
        from stabletts_amd.duration_predictor import DurationPredictor
    cfg = sw.DP_ALL_CASES[case][0]
    m = DurationPredictor(cfg[0], cfg[1], cfg[2], p, cfg[3])
    m.load_state_dict(sw.dp_config_state_dict(case), strict=True)
    return m.cuda()


def _style_ref64(case):
    """(c, loss, gradients) of the float64 restatement, once per case."""
    if case not in _REF64:
        cfg, B, T, spec, seed = sw.STYLE_ALL_CASES[case]
        y, m = sw.style_config_inputs(case)
        _REF64[case] = R.run_style(sw.style_config_state_dict(cfg), y, m, seed, n_head=cfg[4])
    return _REF64[case]


def _dp_ref64(case):
    if case not in _REF64:
        x, m, g = sw.dp_config_inputs(case)
        _REF64[case] = R.run_dp(sw.dp_config_state_dict(case), x, m, g, sw.DP_ALL_CASES[case][4])[:3]
    return _REF64[case]


def _c_err(c, ref):
    assert c.shape == ref.shape and np.isfinite(c).all()
    return float(np.abs(c.astype(np.float64) - ref).max() / np.abs(ref).max())


def _logw_err(lw, ref, mask):
    assert lw.shape == ref.shape and np.isfinite(lw).all()
    assert np.all(lw[mask == 0] == 0.0)                       # exact zeros on padded tokens
    return float(np.abs(lw.astype(np.float64) - ref)[mask > 0].max())


def _check_gradients(gold, case, mod, loss, seed, ref64):
    """Loss and every parameter gradient against the real modules' fixture (its kept elements and norms) and against the
    float64 restatement (every element)."""
    _, loss64, g64 = ref64
    ref_loss = _scalar(gold[f"{case}/loss"])
    e_loss = max(abs(loss - ref_loss) / max(abs(ref_loss), 1.0), abs(loss - loss64) / max(abs(loss64), 1.0))
    grads = {n: p.grad.detach().cpu().numpy() for n, p in mod.named_parameters()}
    assert all(np.isfinite(g).all() for g in grads.values())
    fix = R.digest_errors({k: gold[f"{case}/{k}"] for k in ("names", "norms", "absmax", "full", "sample")}, grads, seed)
    f64 = {}
    for n, g in grads.items():
        ref = g64[n]
        assert g.shape == ref.shape, n
        nr = float(np.linalg.norm(ref))
        f64[n] = (float(np.abs(g.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30)),
                  abs(float(np.linalg.norm(g.astype(np.float64))) - nr) / max(nr, 1e-30))
    wf, w64 = max(fix, key=lambda n: fix[n][0]), max(f64, key=lambda n: f64[n][0])
    print(f"{case}: loss {e_loss:.1e}; gradients vs fixture {fix[wf][0]:.2e} ({wf}), norms {max(e[1] for e in fix.values()):.1e}; "
          f"vs float64 {f64[w64][0]:.2e} ({w64}), norms {max(e[1] for e in f64.values()):.1e}")
    assert e_loss <= LOSS_GATE, (case, loss, ref_loss, loss64)
    bad = {(k, n): e for k, d in (("fixture", fix), ("float64", f64)) for n, e in d.items() if e[0] > GRAD_GATE or e[1] > GRAD_GATE}
    assert not bad, (case, bad)


# ---- 1. inference: c and logw
@pytest.mark.parametrize("case", list(sw.STYLE_ALL_CASES))
def test_style_encoder_inference_matches_reference(gold, case):
    cfg = sw.STYLE_ALL_CASES[case][0]
    y, m = sw.style_config_inputs(case)
    with torch.no_grad():
        c = _style(cfg, train=False)(torch.from_numpy(y).cuda(), torch.from_numpy(m).cuda()).cpu().numpy()
    e_fix, e_64 = _c_err(c, gold[f"{case}/out"]), _c_err(c, _style_ref64(case)[0])
    print(f"{case}: c vs fixture {e_fix:.2e}, vs float64 {e_64:.2e}")
    assert e_fix <= C_GATE and e_64 <= C_GATE


@pytest.mark.parametrize("case", list(sw.DP_ALL_CASES))
def test_duration_predictor_inference_matches_reference(gold, case):
    x, m, g = sw.dp_config_inputs(case)
    with torch.no_grad():
        lw = _dp(case, train=False)(*(torch.from_numpy(a).cuda() for a in (x, m, g))).cpu().numpy()
    e_fix, e_64 = _logw_err(lw, gold[f"{case}/out"], m), _logw_err(lw, _dp_ref64(case)[0], m)
    print(f"{case}: logw vs fixture {e_fix:.2e}, vs float64 {e_64:.2e}")
    assert e_fix <= LOGW_GATE and e_64 <= LOGW_GATE


# ---- 2. training (eval mode: no dropout): the loss and every parameter gradient
@pytest.mark.parametrize("case", list(sw.STYLE_ALL_CASES))
def test_style_encoder_gradients_match_reference(gold, case):
    cfg, B, T, spec, seed = sw.STYLE_ALL_CASES[case]
    y, m = sw.style_config_inputs(case)
    mod = _style(cfg, train=True).eval()
    c = mod(torch.from_numpy(y).cuda(), torch.from_numpy(m).cuda())
    assert c.requires_grad
    loss = (c * R.loss_weights(tuple(c.shape), seed).cuda()).sum()
    loss.backward()
    assert _c_err(c.detach().cpu().numpy(), gold[f"{case}/out"]) <= C_GATE
    _check_gradients(gold, case, mod, loss.item(), seed, _style_ref64(case))


@pytest.mark.parametrize("case", list(sw.DP_ALL_CASES))
def test_duration_predictor_gradients_match_reference(gold, case):
    seed = sw.DP_ALL_CASES[case][4]
    x, m, g = (torch.from_numpy(a).cuda() for a in sw.dp_config_inputs(case))
    mod = _dp(case, train=True).eval()
    logw = mod(x, m, g)
    assert logw.requires_grad
    loss = (logw * R.loss_weights(tuple(logw.shape), seed).cuda()).sum()
    loss.backward()
    with torch.no_grad():
        assert torch.equal(logw.detach(), mod(x, m, g))       # p = 0: the training forward is bitwise the inference forward
    _check_gradients(gold, case, mod, loss.item(), seed, _dp_ref64(case))


# ---- 3. train-mode dropout at a non-default width and head count: the restatement in float64 on the rebuilt masks
def _native_seed(torch_seed):
    torch.manual_seed(torch_seed)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _dropout_errors(mod, loss, loss64, g64, what):
    e_loss = abs(loss - loss64) / max(abs(loss64), 1.0)
    worst = {n: float(np.abs(p.grad.cpu().numpy().astype(np.float64) - g64[n]).max() / max(np.abs(g64[n]).max(), 1e-30))
             for n, p in mod.named_parameters()}
    w = max(worst, key=worst.get)
    print(f"{what}: dropout loss {e_loss:.1e}, gradients vs float64 on the same masks {worst[w]:.2e} ({w})")
    assert e_loss <= LOSS_GATE and worst[w] <= GRAD_GATE, (what, e_loss, worst)


def test_style_encoder_dropout_matches_restatement_with_same_masks():
    case, tseed, p = sw.STYLE_DROPOUT_CASE
    cfg, B, T, spec, seed = sw.STYLE_ALL_CASES[case]
    y, m = sw.style_config_inputs(case)
    mod = _style(cfg, train=True, dropout=p).train()
    w = R.loss_weights((B, cfg[2]), seed).cuda()
    losses = []
    for ts in (tseed, tseed, tseed + 1):
        mod.zero_grad()
        torch.manual_seed(ts)
        loss = (mod(torch.from_numpy(y).cuda(), torch.from_numpy(m).cuda()) * w).sum()
        loss.backward()
        losses.append(loss.item())
        if ts == tseed:
            kept = [p_.grad.clone() for p_ in mod.parameters()]
    assert losses[0] == losses[1] and losses[0] != losses[2]
    drops = R.style_drops(_native_seed(tseed), p, B, cfg[1], T, H=cfg[4])
    for k, d in drops.items():
        assert abs(float((d > 0).float().mean()) - (1.0 - p)) < 0.02, k
    for p_, g_ in zip(mod.parameters(), kept):
        p_.grad = g_
    _, loss64, g64 = R.run_style(sw.style_config_state_dict(cfg), y, m, seed, n_head=cfg[4], drop=drops)
    _dropout_errors(mod, losses[0], loss64, g64, case)


def test_duration_predictor_dropout_matches_restatement_with_same_masks():
    case, tseed, p = sw.DP_DROPOUT_CASE
    cfg, B, T, lengths, seed, wseed = sw.DP_ALL_CASES[case]
    x, m, g = sw.dp_config_inputs(case)
    mod = _dp(case, train=True, p=p).train()
    w = R.loss_weights((B, 1, T), seed).cuda()
    losses = []
    for ts in (tseed, tseed, tseed + 1):
        mod.zero_grad()
        torch.manual_seed(ts)
        loss = (mod(*(torch.from_numpy(a).cuda() for a in (x, m, g))) * w).sum()
        loss.backward()
        losses.append(loss.item())
        if ts == tseed:
            kept = [p_.grad.clone() for p_ in mod.parameters()]
    assert losses[0] == losses[1] and losses[0] != losses[2]
    drops = R.dp_drops(_native_seed(tseed), p, B, cfg[1], T)
    assert abs(float((drops["norm2"] > 0).float().mean()) - (1.0 - p)) < 0.02
    for p_, g_ in zip(mod.parameters(), kept):
        p_.grad = g_
    _, loss64, g64, _ = R.run_dp(sw.dp_config_state_dict(case), x, m, g, seed, drop=drops)
    _dropout_errors(mod, losses[0], loss64, g64, case)


# ---- 4. the split-K weight gradient: which shapes of wgrad_split (synth_weights.wgrad_split) the cases above take
def _wgrad_convs():
    """(case, conv, Cin, Cout, taps, B, T) of every weight gradient the gradient tests above launch (engine_style.cpp /
    engine_duration.cpp: *_train_backward)."""
    for case, (cfg, B, T, _, _) in sw.STYLE_ALL_CASES.items():
        I, Hd, O, K, _ = cfg
        for name, cin, cout, taps in (("fc", Hd, O, 1), ("out_proj", Hd, Hd, 1), ("in_proj", Hd, 3 * Hd, 1), ("temporal", Hd, 2 * Hd, K),
                                      ("spectral.3", Hd, Hd, 1), ("spectral.0", I, Hd, 1)):
            yield case, name, cin, cout, taps, B, T
    for case, (cfg, B, T, _, _, _) in sw.DP_ALL_CASES.items():
        Ci, F, K, G = cfg
        for name, cin, cout, taps, t in (("proj", F, 1, 1, T), ("conv2", F, F, K, T), ("conv1", Ci, F, K, T), ("cond", G, Ci, 1, 1)):
            yield case, name, cin, cout, taps, B, t


def test_split_k_shapes_are_all_covered():
    seen = {}
    for case, name, cin, cout, taps, B, T in _wgrad_convs():
        frames = B * T
        tiles, S, fs, ret, capped = sw.wgrad_split(frames, cin * taps, cout)
        chunks = [(f0, min(f0 + 32, lo + fs, frames) - 1) for lo in range(0, ret * fs, fs) for f0 in range(lo, min(lo + fs, frames), 32)]
        shapes = {"one split": ret == 1, "more than one split, below the cap": 1 < ret < 32, "the 32-split cap": capped and S == 32,
                  "a returned count below the first estimate": ret < S, "a last split shorter than 32 frames": 0 < frames - (ret - 1) * fs < 32 and ret > 1,
                  "a chunk that straddles an item boundary": any(a // T != b // T for a, b in chunks)}
        for k, hit in shapes.items():
            if hit:
                seen.setdefault(k, []).append(f"{case}/{name} ({frames} frames, {tiles} tiles: {ret} x {fs})")
    for k in ("one split", "more than one split, below the cap", "the 32-split cap", "a returned count below the first estimate",
              "a last split shorter than 32 frames", "a chunk that straddles an item boundary"):
        print(f"{k}: {len(seen.get(k, []))} weight gradients, e.g. {seen.get(k, ['-'])[0]}")
        assert seen.get(k), k
    # the two sizes of the repeatability tests, at the default configuration, are among them (now against a reference)
    assert sw.STYLE_ALL_CASES["se_def_b64_t333"][:3] == (sw.STYLE_DEFAULT, 64, 333)
    assert sw.DP_ALL_CASES["dp_def_b64_t200"][:3] == (sw.DP_DEFAULT, 64, 200)
