"""Native spectrogram backward (st_mel_backward) on a real MI355X: the VJP of every case of tests/golden/mel_outputs.npz against
the float64 restatement tests/mel_vjp_restatement.py, silence, the Vocos multi-scale mel loss (vocoders/vocos/models/loss.py)
against tests/golden/mel_loss_grads.npz (tools/make_golden_mel_loss.py), the module rules of stabletts_amd.audio_train and an
8-step Adam trajectory against the same computation in torch on the same GPU.  Every error is printed beside its gate; where torch's
own fp32 error is the yardstick, it is printed too.  Run with ``-m gpu``."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mel_restatement as mr
from tests import mel_vjp_restatement as mv

pytestmark = [pytest.mark.gpu, pytest.mark.grad]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["default", "silence", "tone", "edge_pad1", "edge_hop", "edge_odd"] + [f"ms{n}" for n in (32, 64, 128, 256, 512, 1024, 2048)]
SCALES = list(zip([5, 10, 20, 40, 80, 160, 320], [32, 64, 128, 256, 512, 1024, 2048]))      # loss.py:11


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mel_outputs.npz")))


@pytest.fixture(scope="module")
def loss_gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mel_loss_grads.npz")))


def _modules(sr, n_fft, hop, pad, n_mels):
    from stabletts_amd.audio_train import LinearSpectrogram, LogMelSpectrogram
    lm = LogMelSpectrogram(sr, n_fft, n_fft, hop, 0.0, None, pad, n_mels, False, "reflect", "slaney").cuda()
    lin = LinearSpectrogram(n_fft, n_fft, hop, pad, False, "reflect").cuda()
    return lm, lin


def _native_grad(module, wave, g):
    x = torch.from_numpy(wave).cuda().requires_grad_(True)
    y = module(x)
    y.backward(torch.from_numpy(g).float().cuda())
    return x.grad.cpu().numpy().astype(np.float64)


def _rel(a, ref):
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("case", CASES)
def test_vjp_matches_float64(gold, case):
    sr, n_fft, hop, pad, n_mels = (int(v) for v in gold[case + "/cfg"])
    lm, lin = _modules(sr, n_fft, hop, pad, n_mels)
    wave = gold[case + "/wave"]
    win, fb = lm.spectrogram.window.cpu().numpy(), lm.mel_scale.fb.cpu().numpy()
    rng = np.random.Generator(np.random.PCG64(int.from_bytes(case.encode(), "little") % (1 << 32)))
    mel64 = np.einsum("km,bkt->bmt", fb.astype(np.float64), mr.linear(wave, win, n_fft, hop, pad))      # before the clamp
    for name, module, bank in (("log-mel", lm, fb), ("linear", lin, None)):
        T = mr.frames(wave.shape[1], n_fft, hop, pad)
        g = rng.standard_normal((wave.shape[0], n_mels if bank is not None else n_fft // 2 + 1, T))
        masked = 0
        if bank is not None:            # a clamp-mask flip next to the 1e-5 floor is a property of fp32, not of the kernel
            near = np.abs(mel64 - 1e-5) <= 1e-3 * 1e-5
            masked = int(near.sum())
            g[near] = 0.0
        g = g.astype(np.float32)
        ref = mv.vjp(wave, win, bank, n_fft, hop, pad, g)
        got = _native_grad(module, wave, g)
        xt = torch.from_numpy(wave).requires_grad_(True)
        yt = mv.torch_forward(xt, torch.from_numpy(win), None if bank is None else torch.from_numpy(bank), n_fft, hop, pad)
        (dt,) = torch.autograd.grad(yt, xt, torch.from_numpy(g))
        err, terr = _rel(got, ref), _rel(dt.numpy().astype(np.float64), ref)
        gate = max(1e-4, 2 * terr)
        print(f"{case} {name}: native vs float64 {err:.2e}, torch fp32 vs float64 {terr:.2e} (gate {gate:.1e}); "
              f"g zeroed at {masked} near-floor mels")
        assert got.shape == wave.shape and np.isfinite(got).all() and err <= gate


def test_silence_gives_an_exact_zero_gradient(gold):
    sr, n_fft, hop, pad, n_mels = (int(v) for v in gold["silence/cfg"])
    lm, lin = _modules(sr, n_fft, hop, pad, n_mels)
    wave = gold["silence/wave"]
    rng = np.random.Generator(np.random.PCG64(0))
    T = mr.frames(wave.shape[1], n_fft, hop, pad)
    for module, rows in ((lm, n_mels), (lin, n_fft // 2 + 1)):
        got = _native_grad(module, wave, rng.standard_normal((1, rows, T)).astype(np.float32))
        assert np.isfinite(got).all() and np.all(got == 0.0)


def _multi_scale(module_cls):
    """loss.py:11-20 restated: LogMelSpectrogram(**asdict(MelConfig(n_mels, n_fft, win_length=n_fft, hop_length=n_fft // 4)))
    -- MelConfig's pad is (n_fft - hop) // 2 (config.py:17-19)."""
    return [module_cls(44100, n, n, n // 4, 0.0, None, (n - n // 4) // 2, m, False, "reflect", "slaney").cuda() for m, n in SCALES]


def _loss(mods, x, y):
    return sum(F.l1_loss(m(x), m(y)) for m in mods)


def test_multi_scale_loss_and_gradient_against_the_reference(loss_gold):
    from stabletts_amd.audio_train import LogMelSpectrogram
    mods = _multi_scale(LogMelSpectrogram)
    x = torch.from_numpy(loss_gold["x"]).cuda().requires_grad_(True)
    y = torch.from_numpy(loss_gold["y"]).cuda()
    loss = _loss(mods, x, y)
    loss.backward()
    l64, d64 = float(loss_gold["loss64"].reshape(-1)[0]), loss_gold["dx64"]
    lerr = abs(float(loss.detach()) - l64) / abs(l64)
    lt = abs(float(loss_gold["loss32"].reshape(-1)[0]) - l64) / abs(l64)
    d = x.grad.cpu().numpy().astype(np.float64)
    cos = float((d * d64).sum() / (np.linalg.norm(d) * np.linalg.norm(d64)))
    rl2 = float(np.linalg.norm(d - d64) / np.linalg.norm(d64))
    tl2 = float(np.linalg.norm(loss_gold["dx32"] - d64) / np.linalg.norm(d64))
    print(f"multi-scale loss: native {float(loss.detach()):.7f} vs float64 {l64:.7f}: rel {lerr:.2e}, torch fp32 {lt:.2e} "
          f"(gate {max(1e-5, 2 * lt):.1e});  dL/dx cosine {cos:.7f} (gate 0.9999), rel L2 {rl2:.2e}, torch fp32 {tl2:.2e} "
          f"(gate {max(1e-3, 2 * tl2):.1e})")
    assert x.grad.shape == x.shape == (2, 1, 8192)
    assert lerr <= max(1e-5, 2 * lt) and cos >= 0.9999 and rl2 <= max(1e-3, 2 * tl2)


def test_module_rules():
    from stabletts_amd import _lib
    from stabletts_amd.audio_train import LogMelSpectrogram, LinearSpectrogram
    lm = LogMelSpectrogram(44100, 256, 256, 64, 0.0, None, 96, 40, False, "reflect", "slaney").cuda()
    rng = np.random.Generator(np.random.PCG64(4))
    base = torch.from_numpy((0.3 * rng.standard_normal((3, 1, 5000))).astype(np.float32)).cuda()
    # (B, 1, L) in, (B, 1, L) gradient out; the forward under grad is bitwise the no_grad forward
    x = base.clone().requires_grad_(True)
    y = lm(x)
    with torch.no_grad():
        y0 = lm(base)
    assert torch.equal(y.detach(), y0)
    g = torch.randn_like(y)
    y.backward(g)
    g1 = x.grad.clone()
    assert g1.shape == x.shape and g1.dtype == x.dtype
    # two backward passes are bitwise equal
    x.grad = None
    lm(x).backward(g)
    assert torch.equal(x.grad, g1)
    # a non-contiguous input: same gradient as its contiguous copy
    wide = torch.zeros(3, 10000, device="cuda")
    wide[:, ::2] = base[:, 0]
    xs = wide[:, ::2]
    assert not xs.is_contiguous()
    xs = xs.detach().requires_grad_(True)
    lm(xs).backward(g)
    assert torch.equal(xs.grad, g1[:, 0])
    # y under no_grad and x with grad through the same module in one loss
    xg = base.clone().requires_grad_(True)
    with torch.no_grad():
        yt = lm(0.5 * base)
    F.l1_loss(lm(xg), yt).backward()
    assert torch.isfinite(xg.grad).all() and xg.grad.abs().max() > 0
    # fp16 input: the gradient comes back in the input's dtype
    xh = base.half().requires_grad_(True)
    lm(xh).sum().backward()
    assert xh.grad.dtype == torch.float16 and xh.grad.shape == xh.shape
    # the linear spectrogram too
    lin = LinearSpectrogram(256, 256, 64, 96, False, "reflect").cuda()
    xl = base[:, 0].clone().requires_grad_(True)
    lin(xl).sum().backward()
    assert torch.isfinite(xl.grad).all()
    # ragged stays inference-only under grad
    with pytest.raises(NotImplementedError):
        lm.forward_ragged([base[0, 0].clone().requires_grad_(True)])
    # the C ABI: a bad output value is rejected before any launch
    eng = lm._engine()
    lib = _lib.load()
    w = base[:, 0].contiguous()
    T = lm.frames(5000)
    go = torch.zeros(3, 40, T, device="cuda")
    gx = torch.full((3, 5000), 7.0, device="cuda")
    ws = torch.empty(eng.mel_backward_workspace_bytes(3, 5000), dtype=torch.uint8, device="cuda")
    assert ws.numel() == 3 * T * 256 * 4
    assert lib.st_mel_backward(eng.handle, w.data_ptr(), go.data_ptr(), 3, 5000, 7, gx.data_ptr(), ws.data_ptr(), None) == _lib.ST_ERR_INVALID
    assert lib.st_mel_backward(eng.handle, w.data_ptr(), go.data_ptr(), 3, 96, 0, gx.data_ptr(), ws.data_ptr(), None) == _lib.ST_ERR_INVALID
    assert lib.st_mel_backward(eng.handle, w.data_ptr(), None, 3, 5000, 0, gx.data_ptr(), ws.data_ptr(), None) == _lib.ST_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.all(gx == 7.0)
    # the base class still raises under grad
    from stabletts_amd.audio import LogMelSpectrogram as Base
    with pytest.raises(NotImplementedError):
        Base(44100, 256, 256, 64, 0.0, None, 96, 40, False, "reflect", "slaney").cuda()(base.clone().requires_grad_(True))


def test_adam_trajectory_matches_torch(loss_gold):
    from stabletts_amd.audio_train import LogMelSpectrogram
    mods = _multi_scale(LogMelSpectrogram)
    y = torch.from_numpy(loss_gold["y"]).cuda()

    def torch_loss(x):
        out = 0
        for m in mods:
            win, fb = m.spectrogram.window, m.mel_scale.fb
            a = mv.torch_forward(x.squeeze(1), win, fb, m.n_fft, m.hop_length, m.pad)
            b = mv.torch_forward(y.squeeze(1), win, fb, m.n_fft, m.hop_length, m.pad)
            out = out + F.l1_loss(a, b)
        return out

    losses = {}
    for name, fn in (("native", lambda x: _loss(mods, x, y)), ("torch", torch_loss)):
        x = torch.nn.Parameter(torch.from_numpy(loss_gold["x"]).cuda())
        opt = torch.optim.Adam([x], lr=1e-3)
        ls = []
        for _ in range(8):
            opt.zero_grad()
            loss = fn(x)
            loss.backward()
            opt.step()
            ls.append(float(loss.detach()))
        losses[name] = ls
    rel = [abs(a - b) / abs(b) for a, b in zip(losses["native"], losses["torch"])]
    print("native:", " ".join(f"{v:.5f}" for v in losses["native"]))
    print("torch: ", " ".join(f"{v:.5f}" for v in losses["torch"]))
    print(f"max per-step relative difference {max(rel):.2e} (gate 1e-3)")
    assert max(rel) <= 1e-3 and losses["native"][-1] < losses["native"][0]
