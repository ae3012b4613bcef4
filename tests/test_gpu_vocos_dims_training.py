"""Native Vocos generator training (stabletts_amd.vocos_train) at backbone widths 768 and 1024 and at the configuration the
reference's Vocos trainer builds (vocoders/vocos/config.py:21-26: 128 / 768 / 2048 / 12), on a real MI355X.

The bar is that of tests/test_gpu_vocos_training.py: per tensor the relative L2 distance over the stored elements to the REAL
module's float64 gradients (tests/golden/vocos_dims.npz), at most 4 x the fixture's own fp32-torch-vs-float64 error of that
tensor; shapes the fixture lacks go against the float64 restatement (tests/vocos_vjp_restatement.py, pinned to the real module
at these widths by tests/test_vocos_dims_cpu.py) with 4 x the largest fp32-torch error the fixture records for any parameter.
Every figure is printed beside its bar.  Run with ``-m gpu``.

MEASURED on an MI355X (profiles/vocos_dims_parity.txt; ratio = native error / the fixture's fp32-torch error of the same tensor, bar 4):
  d768     worst parameter 1.16, audio 0.74, d mel 0.87
  d1024    worst parameter 1.00, audio 0.92, d mel 0.90
  trainer  worst parameter 2.19 (head.out.bias: native 6.73e-07, torch fp32 3.08e-07), audio 1.42, d mel 1.14
  vs the float64 restatement (bar 6.64e-06): d768_T1 1.17e-06, d768_R1100 1.14e-06, trainer_width_R260 1.15e-06, d1024_R129 1.20e-06
These are with the GEMMs of the training path in four accumulation chains over K, which the engine uses above dim 512
(SdConvArgs::chains).  As ONE k-ordered chain (what dim 512 keeps) the trainer's case missed the bar on head.out.bias alone, 4.21
(native 1.30e-06), with every other tensor at 2.4 .. 3.9: the chains over K = 768 .. 2050 through 12 blocks were the error.
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import vocos_oracle as vo
from tests import synth_weights as sw
from tests import vocos_dims_cases as D
from tests import vocos_vjp_restatement as R
from tests.test_gpu_vocos_training import _linear_loss, _module, _rel_l2, _run

pytestmark = [pytest.mark.gpu, pytest.mark.grad]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL768 = dict(input_channels=64, dim=768, intermediate_dim=256, num_layers=2)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "vocos_dims.npz")))


def _bar(gold):
    return 4 * max(float(gold[n + "/err32"].max()) for n in D.CASES)


@pytest.mark.parametrize("name", list(D.CASES))
def test_gradients_match_the_reference_module(gold, name):
    """Every parameter, d mel and the audio against the real module's float64 run, each within 4 x torch fp32's own error."""
    fields, B, T, wseed, mseed, _ = D.CASES[name]
    cfg = vo.vocos_config(**fields)
    mod = _module(cfg, vo.make_vocos_state_dict(wseed, cfg))
    W = R.loss_weights((B, T * cfg.hop_length), wseed)
    loss, audio, grads, dmel = _run(mod, vo.make_mel(B, T, mseed, M=cfg.input_channels), _linear_loss(W))
    names = list(gold[name + "/names"])
    assert sorted(grads) == names
    rows = [(n, _rel_l2(D.stored_elements(name, i, grads[n], wseed), gold[f"{name}/grad/{n}"]), float(gold[name + "/err32"][i]))
            for i, n in enumerate(names)]
    rows.append(("audio", _rel_l2(R.sampled(audio, wseed, 1), gold[name + "/audio64"]), float(gold[name + "/audio_err32"])))
    rows.append(("d mel", _rel_l2(dmel, gold[name + "/dmel64"]), float(gold[name + "/dmel_err32"])))
    l64 = float(gold[name + "/loss64"].reshape(-1)[0])
    print(f"{name}: loss {loss:.7f} vs float64 {l64:.7f}; relative L2 to the real module's float64 run (bar: 4 x torch fp32's own)")
    for n, err, own in rows:
        print(f"  {n:42s} native {err:.2e}  torch fp32 {own:.2e}  ratio {err / own:5.2f}")
    worst = max(rows[:-2], key=lambda r: r[1] / r[2])
    print(f"{name}: worst parameter ratio {worst[1] / worst[2]:.2f} ({worst[0]}), audio ratio {rows[-2][1] / rows[-2][2]:.2f}, "
          f"d mel ratio {rows[-1][1] / rows[-1][2]:.2f} (bar 4)")
    assert all(np.isfinite(g).all() for g in grads.values())
    for n, err, own in rows:
        assert err <= 4 * own, (n, err, own)


# id -> (config fields, B, T)
SHAPES = {
    "d768_T1": (SMALL768, 2, 1),                                        # shorter than the depthwise conv's reach
    "d768_R1100": (SMALL768, 25, 44),                                   # FRAME_CASES["R1100"]'s shape: several split-K planes
    "trainer_width_R260": (dict(input_channels=128, dim=768, intermediate_dim=256, num_layers=2), 4, 65),
    "d1024_R129": ({**SMALL768, "dim": 1024}, 3, 43),
}


@functools.lru_cache(maxsize=None)
def _inputs(case):
    fields, B, T = SHAPES[case]
    cfg = vo.vocos_config(**fields)
    return cfg, vo.make_vocos_state_dict(41, cfg), vo.make_mel(B, T, 42, M=cfg.input_channels), R.loss_weights((B, T * cfg.hop_length), 41)


@functools.lru_cache(maxsize=None)
def _native(case):
    cfg, sd, mel, W = _inputs(case)
    mod = _module(cfg, sd)
    _, audio, grads, dmel = _run(mod, mel, _linear_loss(W))
    return mod, audio, grads, dmel


@pytest.mark.parametrize("case", list(SHAPES))
def test_gradients_match_the_float64_restatement(gold, case):
    cfg, sd, mel, W = _inputs(case)
    fields, B, T = SHAPES[case]
    if B * T > 128:       # the weight gradients take several split-K planes (sw.wgrad_split: the Python port of fp32_tile.h's rule)
        planes = {n: sw.wgrad_split(B * T, cin, cout)[3] for n, (cin, cout) in
                  dict(pwconv1=(cfg.dim, cfg.intermediate_dim), pwconv2=(cfg.intermediate_dim, cfg.dim), embed=(7 * cfg.input_channels, cfg.dim)).items()}
        print(f"{case}: R = {B * T}, split-K planes {planes}")
        assert max(planes.values()) > 1
    bar = _bar(gold)
    ref_audio, kept = R.forward(sd, mel, cfg)
    assert np.abs(kept["o"][..., :cfg.n_fft // 2 + 1] - np.log(100.0)).min() > 1e-4      # the two precisions take the same clip branch
    G, ref_dmel = R.backward(sd, kept, W.astype(np.float64), cfg)
    _, audio, grads, dmel = _native(case)
    errs = {n: _rel_l2(grads[n], G[n]) for n in G}
    worst = max(errs, key=errs.get)
    ea, de = _rel_l2(audio, ref_audio), _rel_l2(dmel, ref_dmel)
    print(f"{case}: audio {ea:.2e}, worst parameter {worst} {errs[worst]:.2e}, d mel {de:.2e} (bar {bar:.2e})")
    assert np.isfinite(audio).all() and np.isfinite(dmel).all()
    assert ea <= bar and de <= bar
    for n, e in errs.items():
        assert np.isfinite(grads[n]).all() and e <= bar, (n, e)


def test_two_runs_are_bitwise_equal():
    case = "d768_R1100"
    cfg, sd, mel, W = _inputs(case)
    mod, a1, g1, d1 = _native(case)
    _, a2, g2, d2 = _run(mod, mel, _linear_loss(W))
    assert np.array_equal(a1, a2) and np.array_equal(d1, d2)
    for n in g1:
        assert np.array_equal(g1[n], g2[n]), n


def test_eval_and_no_grad_run_the_inference_path_bitwise():
    from stabletts_amd.vocos import Vocos as Plain
    cfg = vo.vocos_config(**SMALL768)
    sd = vo.make_vocos_state_dict(71, cfg)
    mod, plain = _module(cfg, sd), _module(cfg, sd, Plain)
    mel = torch.from_numpy(vo.make_mel(2, 13, 72, M=64)).cuda()
    with torch.no_grad():
        ref = plain(mel)
        assert torch.equal(mod(mel), ref)
    out = mod.eval()(mel)
    assert not out.requires_grad and torch.equal(out, ref)
    trained = mod.train()(mel)
    assert trained.requires_grad and not torch.equal(trained, ref)      # fp32 training forward: another path, close by
    assert float((trained.detach() - ref).abs().max() / ref.abs().max()) < 1e-3
