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


def duration_predictor_state_dict(seed=DP_SEED, hidden=DP_HIDDEN, filt=DP_FILTER, kernel=DP_KERNEL, gin=GIN):
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
