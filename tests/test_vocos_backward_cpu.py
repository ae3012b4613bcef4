"""CPU checks of the Vocos training path: the float64 restatement of the backward (tests/vocos_vjp_restatement.py) against the
float64 gradients of the REAL reference module (tests/golden/vocos_grads.npz), its clip branch against torch autograd, the
module / install rules that need no device, and the two new C entry points' symbols and host-side argument checks."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import vocos_oracle as vo
from tests import vocos_vjp_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-10         # relative L2 per tensor: both sides are float64 evaluations of the same formulas


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "vocos_grads.npz")))


def _rel_l2(a, ref):
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def _case(name):
    fields, B, T, wseed, mseed, kind = R.CASES[name]
    cfg = vo.vocos_config(**fields)
    return cfg, vo.make_vocos_state_dict(wseed, cfg), vo.make_mel(B, T, mseed, M=cfg.input_channels), wseed, kind


def _mel_loss_grad_float64(audio):
    """d loss / d audio of the multi-scale mel loss (vocoders/vocos/models/loss.py) in float64: torch autograd of the restated
    spectrograms (tests/mel_vjp_restatement.torch_forward) with the drop-in's windows and filter banks."""
    import torch.nn.functional as F
    from stabletts_amd.audio import LogMelSpectrogram
    from tests import mel_vjp_restatement as mv
    y = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "mel_loss_grads.npz"))["y"]).double().squeeze(1)
    x = torch.from_numpy(audio).double().requires_grad_(True)
    loss = 0
    for m, n in zip([5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048]):      # loss.py:11
        mod = LogMelSpectrogram(44100, n, n, n // 4, 0.0, None, (n - n // 4) // 2, m, False, "reflect", "slaney")
        win, fb = mod.spectrogram.window.double(), mod.mel_scale.fb.double()
        loss = loss + F.l1_loss(mv.torch_forward(y, win, fb, n, n // 4, (n - n // 4) // 2),
                                mv.torch_forward(x, win, fb, n, n // 4, (n - n // 4) // 2))
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_the_reference_modules_float64_gradients(gold, name):
    cfg, sd, mel, wseed, kind = _case(name)
    audio, kept = R.forward(sd, mel, cfg)
    if kind == "linear":
        W = R.loss_weights(audio.shape, wseed).astype(np.float64)
        loss, d_audio = float((audio * W).sum()), W
    else:
        loss, d_audio = _mel_loss_grad_float64(audio)
    G, dmel = R.backward(sd, kept, d_audio, cfg)
    names = list(gold[name + "/names"])
    assert names == R.param_names(sd) and sorted(G) == names
    l64 = float(gold[name + "/loss64"].reshape(-1)[0])
    lerr = abs(loss - l64) / abs(l64)
    worst = ("", 0.0)
    for i, n in enumerate(names):
        assert G[n].shape == sd[n].shape
        e = _rel_l2(R.stored_elements(i, G[n], wseed), gold[f"{name}/grad/{n}"])
        worst = max(worst, (n, e), key=lambda v: v[1])
        assert e <= BAR, (n, e)
        assert abs(np.linalg.norm(G[n]) - gold[name + "/norms"][i]) <= 1e-9 * gold[name + "/norms"][i]
    de = _rel_l2(dmel, gold[name + "/dmel64"])
    print(f"{name}: loss rel {lerr:.1e}, worst parameter {worst[0]} {worst[1]:.1e}, d mel {de:.1e} (bar {BAR:.0e})")
    assert lerr <= BAR and de <= BAR


@pytest.fixture(scope="module")
def gold_frames():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "vocos_grads_frames.npz")))


@pytest.mark.parametrize("name", list(R.FRAME_CASES))
def test_restatement_matches_the_reference_modules_float64_gradients_above_128_frames(gold_frames, name):
    """The same pin for the cases of vocos_grads_frames.npz (R = 1100 and the preset at R = 260, where the native weight gradients
    take several split-K planes); d mel and the audio are compared on the fixture's sampled elements.  At 25 x 44 the head's clip
    IS reached: no log-magnitude within 1e-4 of it."""
    gold = gold_frames
    fields, B, T, wseed, mseed, _ = R.FRAME_CASES[name]
    cfg = vo.vocos_config(**fields)
    sd, mel = vo.make_vocos_state_dict(wseed, cfg), vo.make_mel(B, T, mseed, M=cfg.input_channels)
    audio, kept = R.forward(sd, mel, cfg)
    assert np.abs(kept["o"][..., :cfg.n_fft // 2 + 1] - np.log(100.0)).min() > 1e-4
    W = R.loss_weights(audio.shape, wseed).astype(np.float64)
    G, dmel = R.backward(sd, kept, W, cfg)
    names = list(gold[name + "/names"])
    assert names == R.param_names(sd) and sorted(G) == names and len(names) == 9 * cfg.num_layers + 8
    l64 = float(gold[name + "/loss64"].reshape(-1)[0])
    lerr = abs(float((audio * W).sum()) - l64) / abs(l64)
    worst = ("", 0.0)
    for i, n in enumerate(names):
        assert G[n].shape == sd[n].shape
        e = _rel_l2(R.stored_elements(i, G[n], wseed), gold[f"{name}/grad/{n}"])
        worst = max(worst, (n, e), key=lambda v: v[1])
        assert e <= BAR, (n, e)
        assert abs(np.linalg.norm(G[n]) - gold[name + "/norms"][i]) <= 1e-9 * gold[name + "/norms"][i]
    de, ea = _rel_l2(R.sampled(dmel, wseed, 0), gold[name + "/dmel64"]), _rel_l2(R.sampled(audio, wseed, 1), gold[name + "/audio64"])
    print(f"{name}: loss rel {lerr:.1e}, audio {ea:.1e}, worst parameter {worst[0]} {worst[1]:.1e}, d mel {de:.1e} (bar {BAR:.0e})")
    assert lerr <= BAR and de <= BAR and ea <= BAR
    # the fp32 module's own errors, the GPU test's yardsticks: fp32 rounding, not zero and not large
    for k in ("err32", "dmel_err32", "audio_err32"):
        assert 0 < np.min(gold[f"{name}/{k}"]) and np.max(gold[f"{name}/{k}"]) < 1e-4, k
    assert gold[name + "/dmel64"].shape == gold[name + "/audio64"].shape == (R.FRAMES_SAMPLE,)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "vocos_grads_frames.npz")) < 1000 * 1000


def test_fixture_is_what_the_generator_says(gold):
    for name, (fields, B, T, *_rest) in R.CASES.items():
        cfg = vo.vocos_config(**fields)
        assert gold[name + "/dmel64"].shape == (B, cfg.input_channels, T) and gold[name + "/dmel64"].dtype == np.float64
        n = len(gold[name + "/names"])
        assert gold[name + "/err32"].shape == gold[name + "/norms"].shape == gold[name + "/absmax"].shape == (n,)
        assert n == 9 * cfg.num_layers + 8
        # the fp32 module's own error, the GPU test's yardstick: fp32 rounding, not zero and not large
        assert 0 < gold[name + "/err32"].min() and gold[name + "/err32"].max() < 1e-4
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "vocos_grads.npz")) < 1000 * 1000


def _torch_grads(sd, mel, W, cfg):
    p = {k: torch.from_numpy(v).double().requires_grad_(k != "head.istft.window") for k, v in sd.items()}
    m = torch.from_numpy(mel).double().requires_grad_(True)
    audio = R.torch_vocos(p, m, cfg.num_layers)
    (audio * torch.from_numpy(W)).sum().backward()
    return audio.detach().numpy(), {k: v.grad.numpy() for k, v in p.items() if k != "head.istft.window"}, m.grad.numpy()


@pytest.mark.parametrize("T", [1, 3, 9])
def test_clip_branch_and_short_items_match_torch_autograd(T):
    """A head bias raised so that some log-magnitudes pass log(100): d a is exactly 0 there (torch.clip's gradient), everything
    else follows; T = 1 and 3 are shorter than the depthwise conv's reach."""
    cfg = vo.vocos_config(input_channels=64, intermediate_dim=256, num_layers=2)
    sd = vo.make_vocos_state_dict(5, cfg)
    sd["head.out.bias"] = sd["head.out.bias"].copy()
    sd["head.out.bias"][:1025:3] += 4.0
    mel = vo.make_mel(2, T, 6, M=64)
    audio, kept = R.forward(sd, mel, cfg)
    a = kept["o"][..., :1025]
    clipped = np.exp(a) > 100.0
    assert 0.05 < clipped.mean() < 0.6
    W = R.loss_weights(audio.shape, 7).astype(np.float64)
    do = R.istft_head_backward(W, kept["o"], sd["head.istft.window"].astype(np.float64), 2048, 512)
    assert np.all(do[..., :1025][clipped] == 0.0) and np.abs(do[..., :1025][~clipped]).min() > 0
    G, dmel = R.backward(sd, kept, W, cfg)
    ta, tg, tdm = _torch_grads(sd, mel, W, cfg)
    assert _rel_l2(audio, ta) <= BAR and _rel_l2(dmel, tdm) <= BAR
    for n in tg:
        assert _rel_l2(G[n], tg[n]) <= BAR, n


def _cfgs(**over):
    c = vo.vocos_config(**over)
    return (types.SimpleNamespace(input_channels=c.input_channels, dim=c.dim, intermediate_dim=c.intermediate_dim, num_layers=c.num_layers),
            types.SimpleNamespace(n_fft=c.n_fft, hop_length=c.hop_length))


def test_trainable_module_keeps_the_reference_keys_and_asks_for_gradients():
    from stabletts_amd import vocos, vocos_train
    small = dict(input_channels=64, intermediate_dim=256, num_layers=2)
    m = vocos_train.Vocos(*_cfgs(**small))
    base = vocos.Vocos(*_cfgs(**small))
    assert isinstance(m, vocos.Vocos) and m.native_training and not getattr(base, "native_training", False)
    assert list(m.state_dict()) == list(base.state_dict())
    assert all(p.requires_grad for p in m.parameters()) and not any(p.requires_grad for p in base.parameters())
    assert not m.head.istft.window.requires_grad
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vo.make_vocos_state_dict(3, vo.vocos_config(**small)).items()}, strict=True)
    # no CPU fallback, in either mode
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        m(torch.randn(1, 64, 5))
    with torch.no_grad(), pytest.raises(RuntimeError, match="runs only on a HIP device"):
        m(torch.randn(1, 64, 5))


def test_install_vocoder_train_registers_the_trainable_module():
    import stabletts_amd
    from stabletts_amd import vocos, vocos_train
    keys = ("vocoders", "vocoders.vocos", "vocoders.vocos.models", "vocoders.vocos.models.model", "models", "models.flow_matching")
    saved = {k: sys.modules.get(k) for k in keys}
    try:
        stabletts_amd.install(vocoder="train")
        assert sys.modules["vocoders.vocos.models.model"] is vocos_train
        from vocoders.vocos.models.model import Vocos
        assert Vocos is vocos_train.Vocos
        stabletts_amd.install(vocoder=True)
        assert sys.modules["vocoders.vocos.models.model"] is vocos
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_training_entry_points_are_exported_and_check_their_arguments_on_the_host():
    import ctypes
    from stabletts_amd import _lib
    from stabletts_amd.build import build
    build(verbose=False)
    assert "st_vocos_train_forward" in _lib.EXPORTS and "st_vocos_train_backward" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.st_vocos_train_forward.argtypes == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    assert lib.st_vocos_train_backward.argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    # a null handle is ST_ERR_INVALID before anything touches a device
    assert lib.st_vocos_train_forward(None, None, None, 1, 1, None) == _lib.ST_ERR_INVALID
    assert lib.st_vocos_train_backward(None, None, None, None, 1, 1, None) == _lib.ST_ERR_INVALID
    assert lib.st_train_serial(None) == 0
    header = open(os.path.join(ROOT, "include", "stabletts_hip.h")).read()
    assert "int st_vocos_train_forward(" in header and "int st_vocos_train_backward(" in header
