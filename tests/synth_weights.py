"""Seeded weights and inputs of the MelStyleEncoder / DurationPredictor / text-to-mel fixtures (test infrastructure).

numpy PCG64 streams only, so the values do not depend on the torch version; tools/make_golden_synthesise.py (run where the
reference is available) and the GPU tests both import this file, the GPU box never needs the reference.  Distributions follow
PyTorch's default Conv1d / Linear initialisation U(-1/sqrt(fan_in), 1/sqrt(fan_in)) and nn.MultiheadAttention's
xavier_uniform in_proj with zero biases made random, EXCEPT the duration predictor's proj, which is scaled and shifted so that
exp(logw) lands mostly in [1, 12] frames (a realistic duration range; the default init gives durations near 1, where
ceil() decides almost nothing).
"""
import math

import numpy as np
import torch

STYLE_SEED = 7001
# DP seed: chosen by tools/make_golden_synthesise.py so that every valid token of every fixture case keeps its duration
# w = exp(logw) at least MARGIN * w away from an integer (the exact w_ceil / y_lengths checks then test the kernels, not luck)
DP_SEED = 7134
MARGIN = 1e-3
N_MELS, STYLE_HIDDEN, GIN = 128, 128, 256
DP_HIDDEN, DP_FILTER, DP_KERNEL = 256, 1024, 3

# MelStyleEncoder cases: name -> (B, T, lengths or None = unmasked, input seed)
STYLE_CASES = {"se_b1_t1": (1, 1, None, 11), "se_b1_t2600": (1, 2600, None, 12), "se_b3_t37": (3, 37, [37, 20, 5], 13),
               "se_b2_t600": (2, 600, None, 14)}
# DurationPredictor cases: name -> (B, Tx, lengths, input seed)
DP_CASES = {"dp_b3_t37": (3, 37, [37, 25, 9], 21), "dp_b2_t200": (2, 200, [200, 131], 22)}
# full StableTTS.synthesise: B = 2 ragged, CFG 3.0, euler, 6 steps, length_scale 1.2, reference mel of 160 frames
SYNTH = dict(B=2, Tx=29, lengths=[29, 17], T_ref=160, n_steps=6, solver="euler", cfg=3.0, length_scale=1.2, seed=31)


def _u(rng, shape, bound):
    return torch.from_numpy(rng.uniform(-bound, bound, size=shape).astype(np.float32))


def style_encoder_state_dict(seed=STYLE_SEED, n_mels=N_MELS, hidden=STYLE_HIDDEN, gin=GIN, kernel=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    sd["spectral.0.weight"] = _u(rng, (hidden, n_mels), n_mels ** -0.5)
    sd["spectral.0.bias"] = _u(rng, (hidden,), n_mels ** -0.5)
    sd["spectral.3.weight"] = _u(rng, (hidden, hidden), hidden ** -0.5)
    sd["spectral.3.bias"] = _u(rng, (hidden,), hidden ** -0.5)
    for i in range(2):
        b = (hidden * kernel) ** -0.5
        sd[f"temporal.{i}.conv1.weight"] = _u(rng, (2 * hidden, hidden, kernel), b)
        sd[f"temporal.{i}.conv1.bias"] = _u(rng, (2 * hidden,), b)
    sd["slf_attn.in_proj_weight"] = _u(rng, (3 * hidden, hidden), math.sqrt(6.0 / (hidden + 3 * hidden)))
    sd["slf_attn.in_proj_bias"] = _u(rng, (3 * hidden,), 0.1)
    sd["slf_attn.out_proj.weight"] = _u(rng, (hidden, hidden), hidden ** -0.5)
    sd["slf_attn.out_proj.bias"] = _u(rng, (hidden,), 0.1)
    sd["fc.weight"] = _u(rng, (gin, hidden), hidden ** -0.5)
    sd["fc.bias"] = _u(rng, (gin,), hidden ** -0.5)
    return sd


def duration_predictor_state_dict(seed=DP_SEED, hidden=DP_HIDDEN, filt=DP_FILTER, kernel=DP_KERNEL, gin=GIN, kink_free=False):
    """kink_free: conv1 / conv2 weights x 0.1 and their biases +-U(1, 2) per channel, so that every ReLU pre-activation stays
    far from 0 (about half the channels on, half off) and no rounding difference can flip one."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    b1, b2 = (hidden * kernel) ** -0.5, (filt * kernel) ** -0.5
    sd["conv1.weight"] = _u(rng, (filt, hidden, kernel), b1)
    sd["conv1.bias"] = _u(rng, (filt,), b1)
    sd["norm1.weight"] = torch.from_numpy((1.0 + 0.1 * rng.standard_normal(filt)).astype(np.float32))
    sd["norm1.bias"] = torch.from_numpy((0.1 * rng.standard_normal(filt)).astype(np.float32))
    sd["conv2.weight"] = _u(rng, (filt, filt, kernel), b2)
    sd["conv2.bias"] = _u(rng, (filt,), b2)
    sd["norm2.weight"] = torch.from_numpy((1.0 + 0.1 * rng.standard_normal(filt)).astype(np.float32))
    sd["norm2.bias"] = torch.from_numpy((0.1 * rng.standard_normal(filt)).astype(np.float32))
    sd["proj.weight"] = _u(rng, (1, filt, 1), 0.7 * filt ** -0.5)       # logw = N(1.4, ~0.4): w mostly in [1.8, 9]
    sd["proj.bias"] = torch.tensor([1.4], dtype=torch.float32)
    sd["cond.weight"] = _u(rng, (hidden, gin, 1), gin ** -0.5)
    sd["cond.bias"] = _u(rng, (hidden,), gin ** -0.5)
    if kink_free:
        rk = np.random.Generator(np.random.PCG64(seed + 100000))
        for n in ("conv1", "conv2"):
            sd[n + ".weight"] = sd[n + ".weight"] * 0.1
            sign = np.where(rk.random(filt) < 0.5, -1.0, 1.0)
            sd[n + ".bias"] = torch.from_numpy((sign * rk.uniform(1.0, 2.0, size=filt)).astype(np.float32))
    return sd


def mask_of(B, T, lengths):
    m = np.zeros((B, 1, T), np.float32)
    for b, L in enumerate(lengths):
        m[b, 0, :L] = 1.0
    return m


def style_inputs(B, T, lengths, seed, n_mels=N_MELS):
    """Log-mel-like input (mean -5, std 2) and the optional frame mask."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y = (rng.standard_normal((B, n_mels, T)) * 2.0 - 5.0).astype(np.float32)
    return y, (mask_of(B, T, lengths) if lengths is not None else None)


def dp_inputs(B, T, lengths, seed, hidden=DP_HIDDEN, gin=GIN):
    """Text-encoder-like states (masked, as TextEncoder returns them), mask, speaker vectors."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = mask_of(B, T, lengths)
    x = (rng.standard_normal((B, hidden, T)) * m).astype(np.float32)
    g = rng.standard_normal((B, gin)).astype(np.float32)
    return x, m, g


def synth_inputs(n_vocab=401, n_mels=N_MELS, gin=GIN):
    """Token ids (interspersed with 0), lengths, reference mel, CFG parameters (fake_speaker, fake_content), and the
    noise z the decoder starts from (replaces the reference's torch.randn_like, flow_matching.py:45); z has the padded
    mel length, which the fixture's y_lengths fix."""
    s = SYNTH
    rng = np.random.Generator(np.random.PCG64(s["seed"]))
    tok = rng.integers(1, n_vocab, size=(s["B"], s["Tx"])).astype(np.int64)
    tok[:, 0::2] = 0
    for b, L in enumerate(s["lengths"]):
        tok[b, L:] = 0
    y = (rng.standard_normal((s["B"], n_mels, s["T_ref"])) * 2.0 - 5.0).astype(np.float32)
    fake_speaker = (0.5 * rng.standard_normal((1, gin))).astype(np.float32)
    fake_content = (0.5 * rng.standard_normal((1, n_mels, 1))).astype(np.float32)
    return dict(x=tok, x_lengths=np.array(s["lengths"], np.int64), y=y, fake_speaker=fake_speaker, fake_content=fake_content)


def synth_noise(B, n_mels, Ty, seed=SYNTH["seed"] + 1):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((B, n_mels, Ty)).astype(np.float32)


def clears_margin(logw, mask, margin=MARGIN):
    """Every valid token's w = exp(logw) is at least margin * w away from an integer."""
    w = np.exp(logw.astype(np.float64))[mask > 0]
    return bool(np.all(np.abs(w - np.round(w)) >= margin * w))


# ---- the configuration sweep (tests/golden/style_dp_configs.npz, tools/make_golden_style_dp_configs.py) ---------------------
STYLE_DEFAULT = (N_MELS, STYLE_HIDDEN, GIN, 5, 2)           # (n_mels, hidden, out, kernel, heads)
DP_DEFAULT = (DP_HIDDEN, DP_FILTER, DP_KERNEL, GIN)         # (in, filter, kernel, gin)
STYLE_CONFIGS = {"a": (100, 192, 192, 3, 3),    # Cin tail of 4 in a 16-channel chunk, three heads
                 "b": (80, 64, 100, 1, 1),      # one head, partial Cout tile, k 1
                 "c": (128, 256, 256, 5, 4),    # four heads
                 "d": (17, 128, 65, 3, 2)}      # chunk tail of one channel, Cout = tile + 1
DP_CONFIGS = {"a": (192, 128, 5, 192), "b": (256, 768, 1, 100), "c": (100, 256, 3, 256), "d": (24, 128, 3, 17)}
KINK_FREE_ABOVE = 100_000      # ReLU pre-activations on valid tokens (2 sites x filter x tokens) beyond which a case is kink-free


def _rag(T):
    return [T, max(1, 2 * T // 3), max(1, T // 5)]


def _long(B, T):
    """The lengths of the repeatability tests of tests/test_gpu_style_duration_training.py."""
    return [T - (i * 7) % (T // 2) for i in range(B)]


# MelStyleEncoder: name -> (config, B, T, mask, input seed).  mask: a list of lengths, or per item a list of [lo, hi) ranges
# of valid frames.  Every T of {1, 2, 63, 64, 65, 128, 129, 257} occurs; every config sees a T below, at and above a tile edge.
STYLE_CONFIG_CASES = {
    "se_a_t63": (STYLE_CONFIGS["a"], 3, 63, _rag(63), 101), "se_a_t64": (STYLE_CONFIGS["a"], 3, 64, _rag(64), 102),
    "se_a_t65": (STYLE_CONFIGS["a"], 3, 65, _rag(65), 103),
    "se_b_t1": (STYLE_CONFIGS["b"], 3, 1, _rag(1), 104), "se_b_t64": (STYLE_CONFIGS["b"], 3, 64, _rag(64), 105),
    "se_b_t129": (STYLE_CONFIGS["b"], 3, 129, _rag(129), 106),
    "se_c_t2": (STYLE_CONFIGS["c"], 3, 2, _rag(2), 107), "se_c_t128": (STYLE_CONFIGS["c"], 3, 128, _rag(128), 108),
    "se_c_t129": (STYLE_CONFIGS["c"], 3, 129, _rag(129), 109),
    "se_d_t63": (STYLE_CONFIGS["d"], 3, 63, _rag(63), 110), "se_d_t128": (STYLE_CONFIGS["d"], 3, 128, _rag(128), 111),
    "se_d_t257": (STYLE_CONFIGS["d"], 3, 257, _rag(257), 112),
}
# masks no prefix can give, T >= 129: frames 0..69 invalid (the first key tile fully masked), interior holes (one of them a
# whole key tile), a single valid frame (in the first, a middle and the last key tile)
STYLE_MASK_CASES = {
    "se_a_t200_masks": (STYLE_CONFIGS["a"], 3, 200, [[(70, 200)], [(3, 40), (41, 64), (128, 131), (150, 199)], [(77, 78)]], 1121),
    "se_def_t129_masks": (STYLE_DEFAULT, 4, 129, [[(70, 129)], [(0, 1), (5, 9), (64, 65), (127, 128)], [(128, 129)], [(0, 1)]], 2122),
}
# sizes chosen for the split-K weight gradient (with the sweep above: tests/test_gpu_style_duration_configs.py lists the shapes)
STYLE_WGRAD_CASES = {"se_def_b64_t333": (STYLE_DEFAULT, 64, 333, _long(64, 333), 131)}
# DurationPredictor: name -> (config, B, T, lengths, input seed, weight seed).  Cases above KINK_FREE_ABOVE pre-activations take
# the kink-free weights (any seed does: DP_SEED); the others realistic weights whose seed tools/make_golden_style_dp_configs.py
# --search found, so that no float64 ReLU pre-activation of a valid token is within 32 x the fp32-vs-float64 difference of 0.
DP_CONFIG_CASES = {
    "dp_a_t1": (DP_CONFIGS["a"], 3, 1, _rag(1), 141, 7201), "dp_a_t64": (DP_CONFIGS["a"], 3, 64, _rag(64), 142, 7204),
    "dp_a_t129": (DP_CONFIGS["a"], 3, 129, _rag(129), 143, 7341),
    "dp_b_t2": (DP_CONFIGS["b"], 3, 2, _rag(2), 144, 7200), "dp_b_t64": (DP_CONFIGS["b"], 3, 64, _rag(64), 145, DP_SEED),
    "dp_b_t65": (DP_CONFIGS["b"], 3, 65, _rag(65), 1146, DP_SEED),
    "dp_c_t63": (DP_CONFIGS["c"], 3, 63, _rag(63), 147, 7265), "dp_c_t128": (DP_CONFIGS["c"], 3, 128, _rag(128), 148, DP_SEED),
    "dp_c_t257": (DP_CONFIGS["c"], 3, 257, _rag(257), 149, DP_SEED),
    "dp_d_t63": (DP_CONFIGS["d"], 3, 63, _rag(63), 150, 7211), "dp_d_t128": (DP_CONFIGS["d"], 3, 128, _rag(128), 1151, 7213),
    "dp_d_t129": (DP_CONFIGS["d"], 3, 129, _rag(129), 152, 7247),
}
DP_WGRAD_CASES = {"dp_def_b64_t200": (DP_DEFAULT, 64, 200, _long(64, 200), 161, DP_SEED),
                  "dp_d_b16_t257": (DP_CONFIGS["d"], 16, 257, _long(16, 257), 162, DP_SEED)}
# train-mode dropout at a non-default width and head count: case -> (torch seed the native seed is drawn under, p).  The
# predictor's torch seed is the first from 7 under whose masks the ReLU pre-activations keep the margin of the realistic cases
# (tests/test_style_dp_restatement_cpu.py asserts it).
STYLE_DROPOUT_CASE = ("se_a_t65", 5, 0.25)
DP_DROPOUT_CASE = ("dp_c_t63", 7, 0.5)
STYLE_ALL_CASES = {**STYLE_CONFIG_CASES, **STYLE_MASK_CASES, **STYLE_WGRAD_CASES}
DP_ALL_CASES = {**DP_CONFIG_CASES, **DP_WGRAD_CASES}


def dp_kink_free(cfg, lengths):
    return 2 * cfg[1] * sum(lengths) > KINK_FREE_ABOVE


def mask_from_spec(B, T, spec):
    """(B, 1, T) float mask from a list of lengths or a per-item list of [lo, hi) valid ranges."""
    if all(isinstance(v, int) for v in spec):
        return mask_of(B, T, spec)
    m = np.zeros((B, 1, T), np.float32)
    for b, ranges in enumerate(spec):
        for lo, hi in ranges:
            m[b, 0, lo:hi] = 1.0
    return m


def style_config_state_dict(cfg, seed=STYLE_SEED):
    return style_encoder_state_dict(seed, n_mels=cfg[0], hidden=cfg[1], gin=cfg[2], kernel=cfg[3])


def style_config_inputs(case):
    cfg, B, T, spec, seed = STYLE_ALL_CASES[case]
    y, _ = style_inputs(B, T, None, seed, n_mels=cfg[0])
    return y, mask_from_spec(B, T, spec)


def dp_config_state_dict(case):
    cfg, B, T, lengths, seed, wseed = DP_ALL_CASES[case]
    return duration_predictor_state_dict(wseed, hidden=cfg[0], filt=cfg[1], kernel=cfg[2], gin=cfg[3], kink_free=dp_kink_free(cfg, lengths))


def dp_config_inputs(case):
    cfg, B, T, lengths, seed, wseed = DP_ALL_CASES[case]
    return dp_inputs(B, T, lengths, seed, hidden=cfg[0], gin=cfg[3])


# ---- the split-K rule of the fp32 weight gradients ---------------------------------------------------------------------------
def wgrad_split(frames, cin_taps, cout):
    """Python port of wgrad_split (csrc/fp32_tile.h), ONLY for tests to assert which shapes of the split logic their cases reach;
    never a reference for values.  Returns (tiles, count fs was computed from, frames per split, returned count, whether the
    32-split cap cut the count)."""
    tiles = ((cout + 63) // 64) * ((cin_taps + 63) // 64)
    want = min((256 + tiles - 1) // tiles, (frames + 127) // 128)
    S = max(min(want, 32), 1)
    fs = -(-(-(-frames // S)) // 32) * 32
    return tiles, S, fs, -(-frames // fs), want > 32


def wgrad_planes(frames, cin_taps, cout):
    """Planes of one weight-gradient launch (launch_sd_wgrad, launch_pd_wgrad)."""
    return wgrad_split(frames, cin_taps, cout)[3]
