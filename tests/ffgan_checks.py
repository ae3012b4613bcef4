"""Checks of a native FireflyGAN vocoder against float64, shared by its GPU tests (test_gpu_ffgan.py: the default configuration and
the frame-tile edges; test_gpu_ffgan_configs.py: the sweep of its configurations, rates, widths and tile paths) and, for the list
of configurations, by test_ffgan_cpu.py.

Accuracy gate, per compared tensor: e_native = max |native - float64| / max |float64| against e_emul, the same figure of the
float64 restatement (tests/ffgan_restatement.py) with weights and conv / linear inputs rounded to the operand dtype where the
kernels round: e_native <= 2 * e_emul (fp32 accumulation order, roundings that flip at ties; a wrong tap, dilation, halo, phase or
fold is off by order 1), and e_emul < 2e-2 (otherwise the input is ill-conditioned and the gate vacuous).  Every pair is printed.
"""
import functools

import numpy as np
import torch

from tests import ffgan_restatement as R

NAMES = ("audio", "encoder", "pre_tanh")
SMALL = R.small_config()                  # rates (4, 2), kernels (8, 4), resblock kernels (3, 5), dilations ((1, 2), (1, 3)), pre / post 7
DEEP16 = R.small_config(rates=(2, 2), kernels=(4, 4), rk=(11, 3), rd=((5, 1), (1, 2)), c0=64, pre=3, post=5)      # 64 -> 32 -> 16 channels, k = 11, d = 5

# R.small_config() with only the named fields changed (test_gpu_ffgan_configs.py says what each one reaches)
CONFIGS = {
    "small": SMALL,
    "deep16": DEEP16,
    # upsample rates that are no powers of two, and 16: the polyphase packing, the u * Cout row layout and the tiled bias
    "rates_6_10": R.small_config(rates=(6, 10), kernels=(12, 20)),
    "rates_14_2": R.small_config(rates=(14, 2), kernels=(28, 4)),
    "rates_16_12": R.small_config(rates=(16, 12), kernels=(32, 24)),
    # resblock shapes: one pair in one block (X straight into the mean), 4 blocks x 4 dilations with kernel 13 and halo 25
    "one_pair_k1": R.small_config(rk=(1,), rd=((1,),), pre=1, post=1),
    "four_by_four": R.small_config(rates=(2, 2), kernels=(4, 4), rk=(13, 9, 5, 3), rd=((1, 2, 3, 4), (1, 2, 4, 6), (1, 3, 9, 12), (1, 5, 10, 25)),
                                   pre=13, post=13),
    # encoder shapes: widths above 512, 192 mel channels, a narrowing encoder, eight stages, one stage
    "mels192_narrowing": R.small_config(mels=192, dims=(768, 640)),
    "wide_1024_896": R.small_config(dims=(1024, 896)),
    "eight_stages": R.small_config(dims=(128, 256) * 4, depths=(1,) * 8),
    "one_stage": R.small_config(dims=(128,), depths=(5,)),
    # head widths 1024 -> 512 -> 256: 8 and 4 K-chunks per block, conv_post over 256 channels
    "wide_head": R.small_config(rates=(2, 2), kernels=(4, 4), rk=(3,), rd=((1, 2),), c0=1024, dims=(128,), depths=(1,)),
    # hop 2 and a 32-channel head under a 1024-wide encoder: the encoder's GEMMs decide the cost
    "tile_paths": R.small_config(rates=(2,), kernels=(4,), rk=(3,), rd=((1,),), c0=32, dims=(1024, 1024), depths=(1, 1), pre=3, post=3),
    # tests/golden/ffgan_config_outputs.npz
    "ref_a": R.REF_CASES["ref_a"][0],
    "ref_b": R.REF_CASES["ref_b"][0],
}


def build(cfg, dt, seed=R.SEED):
    from stabletts_amd.ffgan import FireflyGANBase
    m = FireflyGANBase(operand_dtype=dt, config=cfg)
    sd = R.make_state_dict(cfg, seed)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), sd


_small = {}


def small_model(name, dt):
    """The native module and its state dict; those of "small" and "deep16", which many tests share, are kept."""
    if name not in ("small", "deep16"):
        return build(CONFIGS[name], dt)
    if (name, dt) not in _small:
        _small[(name, dt)] = build(CONFIGS[name], dt)
    return _small[(name, dt)]


def run_captured(m, mel):
    """-> audio (B, T * hop), encoder (B, D, T), pre_tanh (B, T * hop) as float64 CPU tensors, through debug_capture."""
    B = mel.shape[0]
    eng = m.engine()
    eng.debug_capture(True)
    try:
        audio = m(mel.cuda())
        torch.cuda.synchronize()
        D = m.config["backbone"]["dims"][-1]
        enc = torch.from_numpy(eng.debug_fetch("ffgan.encoder").astype(np.float64)).view(B, -1, D).permute(0, 2, 1)
        pre = torch.from_numpy(eng.debug_fetch("ffgan.pre_tanh").astype(np.float64)).view(B, -1)
    finally:
        eng.debug_capture(False)
    return {"audio": audio.double().cpu(), "encoder": enc, "pre_tanh": pre}


def gate(tag, got, ref, e_emul, names=NAMES):
    bad = []
    for name in names:
        assert tuple(got[name].shape) == tuple(ref[name].shape), (name, got[name].shape, ref[name].shape)
        assert bool(torch.isfinite(got[name]).all()), name
        e_native = R.rel_max(got[name], ref[name])
        print(f"ffgan_parity {tag:<28} {name:<9} e_native {e_native:.3e}   e_emul {e_emul[name]:.3e}")
        assert e_emul[name] < 2e-2, (name, e_emul[name])
        if not e_native <= 2 * e_emul[name]:
            bad.append((name, e_native, e_emul[name]))
    assert not bad, bad


@functools.lru_cache(maxsize=4)
def _float64(name, B, T, mel_seed, items):
    """The state dict, the mel of the whole batch and the float64 restatement of its `items` (None: all): made once, shared by the
    operand dtypes, never written to."""
    cfg = CONFIGS[name]
    sd = R.make_state_dict(cfg, R.SEED)
    mel = R.make_mel(B, T, cfg["backbone"]["input_channels"], mel_seed)
    sub = mel if items is None else mel[list(items)]
    return sd, mel, sub, R.forward(sd, cfg, sub)


def against_restatement(name, dt, B, T, mel_seed, items=None, capture=True):
    """The native module of CONFIGS[name] on make_mel(B, T, ., mel_seed) against the float64 restatement.  items: the utterances that
    are compared (utterances are independent, so the restatement runs on those alone); capture=False runs without debug capture
    and gates the audio only (a batch that runs in chunks refuses the capture)."""
    m, _ = small_model(name, dt)
    cfg = m.config
    items = None if items is None else tuple(items)
    sd, mel, sub, ref = _float64(name, B, T, mel_seed, items)
    em = R.forward(sd, cfg, sub, dt, dt)
    if capture:
        got = run_captured(m, mel)
    else:
        got = {"audio": m(mel.cuda()).cpu().double()}
    names = NAMES if capture else ("audio",)
    if items is not None:
        got = {n: got[n][list(items)] for n in names}
    gate(f"{name} {B}x{T} {dt}", got, ref, {n: R.rel_max(em[n], ref[n]) for n in names}, names)
