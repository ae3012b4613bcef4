"""Native Vocos generator training (stabletts_amd.vocos_train, st_vocos_train_forward / st_vocos_train_backward) on a real MI355X.

Gradients of the three cases of tests/golden/vocos_grads.npz against the REAL module's float64 gradients, per tensor the relative
L2 distance over the stored elements; the bar is 4 x the fixture's own fp32-torch-vs-float64 error of that tensor (both are fp32
evaluations that differ in summation order and in the exp / sin / cos / erf implementations).  Shapes the fixture lacks go
against the float64 restatement (tests/vocos_vjp_restatement.py) with 4 x the largest fp32-torch error the fixture records.
Every figure is printed beside its bar.  Run with ``-m gpu``.

Measured on an MI355X (profiles/vocos_train_parity.txt): see MEASURED below.
"""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vocos_oracle as vo
from tests import vocos_vjp_restatement as R

pytestmark = [pytest.mark.gpu, pytest.mark.grad]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = list(zip([5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048]))      # loss.py:11
SMALL = dict(input_channels=64, intermediate_dim=256, num_layers=2)

# MEASURED (MI355X, profiles/vocos_train_parity.txt; ratio = native error / the fixture's fp32-torch error of the same tensor, bar 4):
#   preset_linear    worst parameter 3.16 (head.out.bias: 1.86e-06 vs torch 5.87e-07; every other tensor 1.8 .. 2.2), d mel 1.86
#   small_linear     worst parameter 1.65, d mel 1.56
#   preset_mel_loss  worst parameter 2.32, d mel 1.88 (8.88e-06 vs torch 4.73e-06)
#   vs the float64 restatement (bar 9.22e-06): T=1 1.76e-06, T=3 1.97e-06, T=61 1.85e-06, B=1 1.93e-06, M=128 2.45e-06, M=192 2.09e-06,
#   clip 1.31e-06, batch vs sum of items 1.92e-07; training waveform vs the real module's 1.4e-06 .. 2.2e-06 (bar 1e-3)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "vocos_grads.npz")))


@pytest.fixture(scope="module")
def loss_gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mel_loss_grads.npz")))


def _cfgs(cfg):
    return (types.SimpleNamespace(input_channels=cfg.input_channels, dim=cfg.dim, intermediate_dim=cfg.intermediate_dim, num_layers=cfg.num_layers),
            types.SimpleNamespace(n_fft=cfg.n_fft, hop_length=cfg.hop_length))


def _module(cfg, sd, cls=None):
    if cls is None:
        from stabletts_amd.vocos_train import Vocos as cls
    m = cls(*_cfgs(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0").train()


def _rel_l2(a, ref):
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def _grads(mod):
    return {n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in mod.named_parameters()}


def _run(mod, mel_np, loss_fn):
    """One generator step's forward and backward -> (loss, audio, {name: grad}, d mel), numpy."""
    mod.zero_grad(set_to_none=True)
    mel = torch.from_numpy(mel_np).cuda().requires_grad_(True)
    audio = mod(mel)
    loss = loss_fn(audio)
    loss.backward()
    return float(loss.detach()), audio.detach().cpu().numpy(), _grads(mod), mel.grad.cpu().numpy().astype(np.float64)


def _linear_loss(W):
    Wt = torch.from_numpy(W).cuda()
    return lambda audio: (audio * Wt).sum()


def _multi_scale():
    """loss.py:11-20 with the native trainable spectrograms (stabletts_amd.audio_train)."""
    from stabletts_amd.audio_train import LogMelSpectrogram
    return [LogMelSpectrogram(44100, n, n, n // 4, 0.0, None, (n - n // 4) // 2, m, False, "reflect", "slaney").cuda() for m, n in SCALES]


def _check_against_fixture(gold, name, grads, dmel, wseed):
    names = list(gold[name + "/names"])
    assert sorted(grads) == names
    worst, lines = 0.0, []
    for i, n in enumerate(names):
        err = _rel_l2(R.stored_elements(i, grads[n], wseed), gold[f"{name}/grad/{n}"])
        own = float(gold[name + "/err32"][i])
        worst = max(worst, err / own)
        lines.append(f"  {n:42s} native {err:.2e}  torch fp32 {own:.2e}  ratio {err / own:5.2f}")
    de, down = _rel_l2(dmel, gold[name + "/dmel64"]), float(gold[name + "/dmel_err32"])
    print(f"{name}: relative L2 to the real module's float64 gradients (bar: 4 x torch fp32's own)")
    print("\n".join(lines))
    print(f"  {'d mel':42s} native {de:.2e}  torch fp32 {down:.2e}  ratio {de / down:5.2f}")
    print(f"{name}: worst parameter ratio {worst:.2f}, d mel ratio {de / down:.2f} (bar 4)")
    for i, n in enumerate(names):
        assert np.isfinite(grads[n]).all()
        assert _rel_l2(R.stored_elements(i, grads[n], wseed), gold[f"{name}/grad/{n}"]) <= 4 * float(gold[name + "/err32"][i]), n
    assert de <= 4 * down


@pytest.mark.parametrize("name", ["preset_linear", "small_linear"])
def test_gradients_match_the_reference_module(gold, name):
    fields, B, T, wseed, mseed, _ = R.CASES[name]
    cfg = vo.vocos_config(**fields)
    sd = vo.make_vocos_state_dict(wseed, cfg)
    mod = _module(cfg, sd)
    W = R.loss_weights((B, T * cfg.hop_length), wseed)
    loss, audio, grads, dmel = _run(mod, vo.make_mel(B, T, mseed, M=cfg.input_channels), _linear_loss(W))
    l64 = float(gold[name + "/loss64"].reshape(-1)[0])
    print(f"{name}: loss {loss:.7f} vs float64 {l64:.7f} (rel {abs(loss - l64) / abs(l64):.2e}; torch fp32 "
          f"{abs(float(gold[name + '/loss32'].reshape(-1)[0]) - l64) / abs(l64):.2e})")
    _check_against_fixture(gold, name, grads, dmel, wseed)


def test_generator_step_with_the_native_mel_loss_matches_the_reference(gold, loss_gold):
    """Case 3 end to end: mel -> Vocos -> seven-scale log-mel L1 loss -> backward, every kernel between the mel and the gradients
    native (vocoders/vocos/train.py:94,115,128)."""
    name = "preset_mel_loss"
    fields, B, T, wseed, mseed, _ = R.CASES[name]
    cfg = vo.vocos_config(**fields)
    mod = _module(cfg, vo.make_vocos_state_dict(wseed, cfg))
    mods = _multi_scale()
    y = torch.from_numpy(loss_gold["y"]).cuda()
    loss, audio, grads, dmel = _run(mod, vo.make_mel(B, T, mseed), lambda a: sum(F.l1_loss(m(y), m(a.unsqueeze(1))) for m in mods))
    l64, l32 = float(gold[name + "/loss64"].reshape(-1)[0]), float(gold[name + "/loss32"].reshape(-1)[0])
    lerr, lt = abs(loss - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    # the loss gate of tests/test_gpu_mel_backward.py's multi-scale test: max(1e-5, 2 x torch fp32's own error)
    print(f"{name}: loss {loss:.7f} vs float64 {l64:.7f}: rel {lerr:.2e}, torch fp32 {lt:.2e} (gate {max(1e-5, 2 * lt):.1e})")
    assert lerr <= max(1e-5, 2 * lt)
    _check_against_fixture(gold, name, grads, dmel, wseed)


def _restatement(cfg, sd, mel, W):
    audio, kept = R.forward(sd, mel, cfg)
    G, dmel = R.backward(sd, kept, W.astype(np.float64), cfg)
    return audio, G, dmel


@pytest.mark.parametrize("B,T,over", [(2, 1, {}), (2, 3, {}), (2, 61, {}), (1, 20, {}), (2, 9, dict(input_channels=128)),
                                      (2, 9, dict(input_channels=192))],
                         ids=["T1", "T3", "T61", "B1", "M128", "M192"])
def test_gradients_match_the_float64_restatement_at_other_shapes(gold, B, T, over):
    """T = 1 and 3 are shorter than the depthwise conv's reach, T = 61 leaves a ragged 64-frame tile, the SMALL config has
    input_channels 64.  Bar: 4 x the largest fp32-torch-vs-float64 error the fixture records for any tensor."""
    bar = 4 * max(float(gold[n + "/err32"].max()) for n in R.CASES)
    cfg = vo.vocos_config(**{**SMALL, **over})
    sd = vo.make_vocos_state_dict(41, cfg)
    mel = vo.make_mel(B, T, 42, M=cfg.input_channels)
    W = R.loss_weights((B, T * cfg.hop_length), 43)
    ref_audio, G, ref_dmel = _restatement(cfg, sd, mel, W)
    _, audio, grads, dmel = _run(_module(cfg, sd), mel, _linear_loss(W))
    errs = {n: _rel_l2(grads[n], G[n]) for n in G}
    worst = max(errs, key=errs.get)
    ea, de = _rel_l2(audio, ref_audio), _rel_l2(dmel, ref_dmel)
    print(f"B={B} T={T} M={cfg.input_channels}: audio {ea:.2e}, worst parameter {worst} {errs[worst]:.2e}, d mel {de:.2e} (bar {bar:.2e})")
    assert ea <= bar and de <= bar
    for n, e in errs.items():
        assert e <= bar, (n, e)


def test_two_runs_are_bitwise_equal_and_items_do_not_mix(gold):
    bar = 4 * max(float(gold[n + "/err32"].max()) for n in R.CASES)
    cfg = vo.vocos_config(**SMALL)
    sd = vo.make_vocos_state_dict(51, cfg)
    B, T = 3, 37
    mel = vo.make_mel(B, T, 52, M=64)
    W = R.loss_weights((B, T * cfg.hop_length), 53)
    mod = _module(cfg, sd)
    _, a1, g1, d1 = _run(mod, mel, _linear_loss(W))
    _, a2, g2, d2 = _run(mod, mel, _linear_loss(W))
    assert np.array_equal(a1, a2) and np.array_equal(d1, d2)
    for n in g1:
        assert np.array_equal(g1[n], g2[n]), n
    # an item alone: the same waveform and d mel bit for bit; the parameter gradients of the batch are the sum of the items'
    total = {n: np.zeros_like(v) for n, v in g1.items()}
    for b in range(B):
        _, ab, gb, db = _run(mod, mel[b:b + 1], _linear_loss(W[b:b + 1]))
        assert np.array_equal(ab[0], a1[b]) and np.array_equal(db[0], d1[b]), b
        for n in gb:
            total[n] += gb[n]
    errs = {n: _rel_l2(g1[n], total[n]) for n in g1}
    worst = max(errs, key=errs.get)
    print(f"batch vs sum of items: worst {worst} {errs[worst]:.2e} (bar {bar:.2e})")
    assert errs[worst] <= bar


def test_clipped_magnitudes_get_an_exactly_zero_gradient(gold):
    """head.py:107: torch.clip(max=100) passes no gradient where exp(a) > 100.  Bins whose bias is raised by 20 are clipped in every
    frame: their log-magnitude rows of head.out get exactly 0; bins raised by 4 are clipped in some frames; the rest follows the
    restatement."""
    bar = 4 * max(float(gold[n + "/err32"].max()) for n in R.CASES)
    cfg = vo.vocos_config(**SMALL)
    sd = vo.make_vocos_state_dict(61, cfg)
    sd["head.out.bias"] = sd["head.out.bias"].copy()
    sd["head.out.bias"][0:1025:8] += 20.0
    sd["head.out.bias"][3:1025:8] += 4.0
    B, T = 2, 11
    mel = vo.make_mel(B, T, 62, M=64)
    W = R.loss_weights((B, T * cfg.hop_length), 63)
    ref_audio, G, ref_dmel = _restatement(cfg, sd, mel, W)
    _, kept = R.forward(sd, mel, cfg)
    clipped = np.exp(kept["o"][..., :1025]) > 100.0
    assert clipped[..., 0::8].all() and 0 < clipped[..., 3::8].mean() < 1 and not clipped[..., 1::8].any()
    # no log-magnitude sits within fp32 rounding of the clip, where the two precisions could disagree about the branch
    assert np.abs(kept["o"][..., :1025] - np.log(100.0)).min() > 1e-4
    _, audio, grads, dmel = _run(_module(cfg, sd), mel, _linear_loss(W))
    assert np.all(grads["head.out.bias"][0:1025:8] == 0.0) and np.all(grads["head.out.weight"][0:1025:8] == 0.0)
    assert np.all(grads["head.out.bias"][1025:] != 0.0)          # the phases of clipped bins still get their gradient
    errs = {n: _rel_l2(grads[n], G[n]) for n in G}
    worst = max(errs, key=errs.get)
    print(f"clip: audio {_rel_l2(audio, ref_audio):.2e}, worst parameter {worst} {errs[worst]:.2e}, d mel {_rel_l2(dmel, ref_dmel):.2e} (bar {bar:.2e})")
    assert errs[worst] <= bar and _rel_l2(dmel, ref_dmel) <= bar


def test_training_waveform_is_inside_the_inference_gate():
    """The fp32 training forward against the REAL module's waveforms (tests/golden/vocos_outputs.npz), in the inference test's
    metric and inside its 1e-3 bar (tests/test_gpu_vocos.py) -- far inside: no 16-bit operand anywhere."""
    from oracle.make_golden_vocos import CASES, SD_SEED
    g = np.load(os.path.join(ROOT, "tests", "golden", "vocos_outputs.npz"))
    mod = _module(vo.VocosConfig, vo.make_vocos_state_dict(SD_SEED))
    for name, (B, T, seed) in CASES.items():
        audio = mod(torch.from_numpy(vo.make_mel(B, T, seed)).cuda())
        assert audio.requires_grad and audio.shape == g[name + ".audio"].shape
        e = float(np.abs(audio.detach().cpu().numpy() - g[name + ".audio"]).max() / np.abs(g[name + ".audio"]).max())
        print(f"training forward {name}: audio {e:.2e} (bar 1e-3)")
        assert e < 1e-3


def test_module_rules():
    from stabletts_amd import _lib
    from stabletts_amd.vocos import Vocos as Plain
    cfg = vo.vocos_config(**SMALL)
    sd = vo.make_vocos_state_dict(71, cfg)
    mod = _module(cfg, sd)
    plain = _module(cfg, sd, Plain)
    mel = torch.from_numpy(vo.make_mel(2, 13, 72, M=64)).cuda()
    # under no_grad and in eval mode: the inference path, bitwise the plain module's
    with torch.no_grad():
        ref = plain(mel)
        assert torch.equal(mod(mel), ref)
    out = mod.eval()(mel)
    assert not out.requires_grad and torch.equal(out, ref)
    mod.train()
    # the plain module still refuses to train
    plain.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="inference-only"):
        plain(mel)
    # a (B, 1, L) consumer, .detach() (train.py:94,98), clip_grad_norm_, parameter hooks (what DDP installs)
    fired = []
    hooks = [p.register_hook(lambda g, n=n: fired.append(n)) for n, p in mod.named_parameters()]
    fake = mod(mel).unsqueeze(1)
    assert fake.shape == (2, 1, 13 * 512) and fake.requires_grad and not fake.detach().requires_grad
    fake.square().mean().backward()
    for h in hooks:
        h.remove()
    assert sorted(fired) == sorted(n for n, _ in mod.named_parameters())
    assert all(p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all() for p in mod.parameters())
    norm = torch.nn.utils.clip_grad_norm_(mod.parameters(), 1000)
    assert torch.isfinite(norm) and norm > 0
    assert mod.head.istft.window.grad is None
    # a mel that requires grad gets its gradient, in its shape
    m2 = mel.clone().requires_grad_(True)
    mod(m2).sum().backward()
    assert m2.grad.shape == m2.shape and torch.isfinite(m2.grad).all() and m2.grad.abs().max() > 0
    # a second backward through the same forward is refused
    a = mod(mel)
    a.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="differentiated already"):
        a.sum().backward()
    # another training forward in between: the first one's activations are gone
    a = mod(mel)
    mod(mel)
    with pytest.raises(RuntimeError, match="activations are gone"):
        a.sum().backward()
    # an optimizer step, then inference: the packed copies follow the new weights
    opt = torch.optim.SGD(mod.parameters(), lr=1e-2)
    mod.zero_grad()
    mod(mel).square().mean().backward()
    opt.step()
    with torch.no_grad():
        after = mod(mel)
        plain.load_state_dict(mod.state_dict())
        assert not torch.equal(after, ref) and torch.equal(after, plain(mel))
    # the C ABI: bad sizes, null pointers, a backward that is not the held forward's
    eng, lib = mod.engine(), _lib.load()
    x = mel.contiguous()
    audio = torch.full((2, 13 * 512), 7.0, device="cuda")
    flat = torch.full((eng.grad_layout()[None],), 7.0, device="cuda")
    assert lib.st_vocos_train_forward(eng.handle, x.data_ptr(), audio.data_ptr(), 0, 13, None) == _lib.ST_ERR_INVALID
    assert lib.st_vocos_train_forward(eng.handle, x.data_ptr(), audio.data_ptr(), 2, 0, None) == _lib.ST_ERR_INVALID
    assert lib.st_vocos_train_forward(eng.handle, None, audio.data_ptr(), 2, 13, None) == _lib.ST_ERR_INVALID
    assert lib.st_vocos_train_forward(eng.handle, x.data_ptr(), audio.data_ptr(), 1 << 20, 1 << 10, None) == _lib.ST_ERR_INVALID
    assert lib.st_vocos_train_backward(eng.handle, audio.data_ptr(), None, None, 2, 13, None) == _lib.ST_ERR_INVALID
    eng.finalize()                                                   # drops the held activations
    assert eng.train_serial() == 0
    assert lib.st_vocos_train_backward(eng.handle, audio.data_ptr(), None, flat.data_ptr(), 2, 13, None) == _lib.ST_ERR_STATE
    assert b"st_vocos_train_forward" in lib.st_last_error(eng.handle)
    assert lib.st_vocos_train_forward(eng.handle, x.data_ptr(), audio.data_ptr(), 2, 13, None) == _lib.ST_OK
    assert lib.st_vocos_train_backward(eng.handle, audio.data_ptr(), None, flat.data_ptr(), 2, 12, None) == _lib.ST_ERR_STATE
    torch.cuda.synchronize()
    assert torch.all(flat == 7.0) and torch.isfinite(audio).all()
    dec = _lib.Engine(128, 256, 1024, 4, 6, 3, 256, "f16", 0)       # a handle of another kind
    assert lib.st_vocos_train_forward(dec.handle, x.data_ptr(), audio.data_ptr(), 2, 13, None) == _lib.ST_ERR_STATE
    dec.close()


def test_adamw_steps_track_torch_autograd(loss_gold):
    """Six steps of the generator's optimizer (vocoders/vocos/train.py:73: AdamW, lr = TrainConfig.learning_rate = 1e-4, default
    betas; clip_grad_norm_ 1000 as train.py:130) on the native path against torch autograd of the same forward written in torch
    ops (vocos_vjp_restatement.torch_vocos) on the same GPU, both under the native multi-scale mel loss; gated as the trajectory
    test of tests/test_gpu_mel_backward.py: per-step relative loss difference <= 1e-3, and the loss goes down.
    From random weights the trajectory amplifies rounding: the torch leg started from weights moved by one fp32 ulp is 1.4e-4
    from itself at step 6, the native leg 1.1e-4 to 2.6e-4 from torch over three runs (the torch leg's backward does not repeat
    bitwise; profiles/vocos_train_parity.txt)."""
    cfg = vo.VocosConfig
    sd = vo.make_vocos_state_dict(81)
    mods = _multi_scale()
    y = torch.from_numpy(loss_gold["y"]).cuda()
    mel = torch.from_numpy(vo.make_mel(2, 16, 82)).cuda()
    loss_of = lambda a: sum(F.l1_loss(m(y), m(a.unsqueeze(1))) for m in mods)      # noqa: E731
    native = _module(cfg, sd)
    tp = {k: torch.nn.Parameter(torch.from_numpy(v).cuda(), requires_grad=k != "head.istft.window") for k, v in sd.items()}
    runs = {"native": (lambda: native(mel), list(native.parameters())),
            "torch": (lambda: R.torch_vocos(tp, mel, cfg.num_layers), [p for p in tp.values() if p.requires_grad])}
    losses = {}
    for name, (fwd, params) in runs.items():
        opt = torch.optim.AdamW(params, lr=1e-4)
        ls = []
        for _ in range(6):
            opt.zero_grad()
            loss = loss_of(fwd())
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, 1000)
            opt.step()
            ls.append(float(loss.detach()))
        losses[name] = ls
    rel = [abs(a - b) / abs(b) for a, b in zip(losses["native"], losses["torch"])]
    print("native:", " ".join(f"{v:.5f}" for v in losses["native"]))
    print("torch: ", " ".join(f"{v:.5f}" for v in losses["torch"]))
    print(f"max per-step relative difference {max(rel):.2e} (gate 1e-3)")
    assert max(rel) <= 1e-3 and losses["native"][-1] < losses["native"][0]
