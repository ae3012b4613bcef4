"""Generates tests/golden/mrd_grads.npz: feature maps and gradients of the REAL reference multi-resolution discriminator
(vocoders/vocos/models/discriminator.py, unmodified, CPU, one thread) under torch autograd, for the native discriminator
(stabletts_amd/discriminator.py).  Run where a checkout of the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_mrd.py

The reference module builds torchaudio's ``Spectrogram(n_fft=W, hop_length=W // 4, win_length=W, power=None)``.  torchaudio is not
needed here: a local stand-in ``torchaudio.transforms.Spectrogram`` is installed first, which is the call that transform makes,
``torch.stft(x, W, hop_length=W // 4, win_length=W, window=hann_window(W), center=True, pad_mode="reflect", normalized=False,
onesided=True, return_complex=True)``, with the window a persistent buffer as torchaudio registers it (so the stand-in's
``state_dict`` has torchaudio's ``spec_fn.window`` entry).  The tool asserts that this stand-in agrees with the direct float64 DFT of
tests/mrd_restatement.py to float64 rounding.

The two linear cases need slope 1.0 where the reference hard-codes ``leaky_relu(band, 0.1)`` (discriminator.py:163): for these two
cases only, ``torch.nn.functional.leaky_relu`` is replaced by the identity while the module runs, and restored afterwards.  No
reference file is edited.

Weights and audio: tests/mrd_restatement.py (make_dr_state_dict / make_mrd_state_dict, mpd_restatement.make_audio).  Every case
runs twice, the module in fp32 and in float64.  Stored from the float64 run, per tensor as mrd_restatement.stored keeps it
(whole up to 512 elements, else 256 fixed sampled elements); from the fp32 run only err32, the relative L2 distance of the
stored elements from the float64 ones -- the yardstick of the GPU tests.

  linear_w32 / linear_w128  DiscriminatorR(W) with every leaky ReLU of slope 1.0, (B, T) = (2, 97) / (3, 331), loss =
                            sum_fmaps sum(fmap * W), W seeded: exactly linear, no branch.  names, shapes, fmap_shapes, fmap/<i>,
                            fmap_err32, grad/<name>, err32, dx64 (whole), dx_err32, loss64, state_names / state_shapes (the state_dict).
  train_step                MultiResolutionDiscriminator(), B = 2, T = 2100, loss = discriminator_loss + feature_loss +
                            generator_loss (loss.py:37-66) on (y, y_hat), y_hat requiring grad.  The first seed of
                            mrd_restatement.TRAIN_STEP["seeds"] whose fp32 and float64 runs agree in EVERY sign -- every leaky-ReLU
                            output of every layer and every rl - gl -- is taken, and that is asserted, so no branch flip
                            contaminates err32.  names, shapes, state_names, state_shapes, seed, losses64 / losses32 (disc, feat, gen), grad/<name>, err32,
                            dyhat64 (whole), dyhat_err32, fmap/<resolution index>/<i> (of cat([y, y_hat])), fmap_err32,
                            logits/<resolution index> (whole).
Fixed zip timestamps: regenerating the file reproduces it byte for byte (asserted by writing it twice).
"""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mrd_grads.npz")


def _install_torchaudio_standin():
    """tools/make_golden_mel.py's stand-in (loss.py imports utils.audio, which needs MelScale) plus a Spectrogram that is the
    torch.stft call of torchaudio's transform, as an importable ``torchaudio.transforms``."""
    from make_golden_mel import _install_torchaudio_standin as base
    base()

    class Spectrogram(torch.nn.Module):
        def __init__(self, n_fft, hop_length, win_length, power):
            super().__init__()
            assert power is None and win_length == n_fft
            self.n_fft, self.hop_length = n_fft, hop_length
            self.register_buffer("window", torch.hann_window(n_fft))          # persistent, as torchaudio registers it

        def forward(self, x):
            return torch.stft(x, self.n_fft, hop_length=self.hop_length, win_length=self.n_fft, window=self.window.to(x.dtype), center=True,
                              pad_mode="reflect", normalized=False, onesided=True, return_complex=True)

    ta = sys.modules["torchaudio"]
    tr = types.ModuleType("torchaudio.transforms")
    tr.MelScale = ta.transforms.MelScale
    tr.Spectrogram = Spectrogram
    ta.transforms = tr
    sys.modules["torchaudio.transforms"] = tr


def _load(ref_dir, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_dir, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _SlopeOne:
    """While active, torch.nn.functional.leaky_relu is the identity (slope 1.0): the linear cases."""
    def __enter__(self):
        self.saved = torch.nn.functional.leaky_relu
        torch.nn.functional.leaky_relu = lambda x, negative_slope=0.01, inplace=False: x
        return self

    def __exit__(self, *a):
        torch.nn.functional.leaky_relu = self.saved


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE")
    if not ref_dir or not os.path.isfile(os.path.join(ref_dir, "vocoders", "vocos", "models", "discriminator.py")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    torch.set_num_threads(1)
    from make_golden_mel import _save
    from tests import mrd_restatement as R
    _install_torchaudio_standin()
    disc = _load(ref_dir, ("vocoders", "vocos", "models", "discriminator.py"), "ref_vocos_discriminator")      # reference, unmodified
    sys.path.insert(0, ref_dir)
    loss_mod = _load(ref_dir, ("vocoders", "vocos", "models", "loss.py"), "ref_vocos_loss")                    # reference, unmodified

    # the stand-in Spectrogram against the restatement's direct DFT, float64
    for W, T in ((32, 97), (128, 331), (512, 2100), (2048, 2100)):
        x = torch.from_numpy(R.make_audio(2, T, 7 + W)).double()
        d = disc.DiscriminatorR(W).double()
        got = torch.cat(d.spectrogram(x), dim=-1)
        err = R.rel_l2(got.numpy(), R.spectrum(x, W).numpy())
        print(f"stand-in Spectrogram vs direct DFT, W = {W}: {err:.2e}")
        assert got.shape == (2, 2, 1 + T // (W // 4), W // 2 + 1) and err <= 1e-12

    res = {}

    def t(a, dt):
        return torch.from_numpy(a).to(dt)

    # ---- linear cases
    for case, (W, B, T, wseed, aseed) in R.LINEAR_CASES.items():
        sd, x_np = R.make_dr_state_dict(wseed), R.make_audio(B, T, aseed)
        runs = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            d = disc.DiscriminatorR(W)
            d.load_state_dict({k: torch.from_numpy(v) for k, v in R.with_windows(sd, W).items()}, strict=True)
            d = d.to(dt)
            x = t(x_np, dt).requires_grad_(True)
            with _SlopeOne():
                logits, fmap = d(x)
            assert logits is fmap[-1] and len(fmap) == 21
            loss = R.linear_loss(fmap, wseed)
            loss.backward()
            runs[tag] = (float(loss), [f.detach().numpy() for f in fmap], {n: q.grad.numpy() for n, q in d.named_parameters()}, x.grad.numpy())
        (l64, f64, g64, dx64), (l32, f32, g32, dx32) = runs["64"], runs["32"]
        names = list(sd)
        assert names == list(g64) == [n for n, _ in d.named_parameters()]
        res[f"{case}/names"] = np.array(names)
        res[f"{case}/shapes"] = np.array([",".join(map(str, sd[n].shape)) for n in names])
        res[f"{case}/state_names"] = np.array(list(d.state_dict()))          # the parameters and spec_fn.window
        res[f"{case}/state_shapes"] = np.array([",".join(map(str, v.shape)) for v in d.state_dict().values()])
        assert list(d.state_dict()) == list(R.with_windows(sd, W)) and len(d.state_dict()) == 79
        res[f"{case}/loss64"] = np.float64(l64)
        res[f"{case}/fmap_shapes"] = np.array([",".join(map(str, f.shape)) for f in f64])
        ferr = []
        for i, (a, b) in enumerate(zip(f32, f64)):
            res[f"{case}/fmap/{i}"] = R.stored(1000 + i, b, wseed)
            ferr.append(R.rel_l2(R.stored(1000 + i, a, wseed), res[f"{case}/fmap/{i}"]))
        res[f"{case}/fmap_err32"] = np.array(ferr)
        err = []
        for i, n in enumerate(names):
            res[f"{case}/grad/{n}"] = R.stored(i, g64[n], wseed)
            err.append(R.rel_l2(R.stored(i, g32[n], wseed), res[f"{case}/grad/{n}"]))
        res[f"{case}/err32"] = np.array(err)
        res[f"{case}/dx64"] = dx64
        res[f"{case}/dx_err32"] = np.float64(R.rel_l2(dx32, dx64))
        print(case, "fp32 vs float64: loss", abs(l32 - l64) / abs(l64), "fmaps max", max(ferr), "min", min(ferr), "grad max", max(err), "min", min(err),
              "dx", float(res[f"{case}/dx_err32"]))

    # ---- train_step
    ts = R.TRAIN_STEP
    B, T = ts["B"], ts["T"]
    chosen = None
    for seed in ts["seeds"]:
        sd = R.make_mrd_state_dict(seed)
        y_np, yh_np = R.make_audio(B, T, seed + 1), R.make_audio(B, T, seed + 2)
        runs = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            m = disc.MultiResolutionDiscriminator()
            m.load_state_dict({k: torch.from_numpy(v) for k, v in R.with_windows(sd).items()}, strict=True)
            m = m.to(dt)
            pre0 = []
            hooks = [stack[0].register_forward_hook(lambda mod, i, o: pre0.append(o.detach().clone())) for d in m.discriminators for stack in d.band_convs]
            y, yh = t(y_np, dt), t(yh_np, dt).requires_grad_(True)
            y_d_rs, y_d_gs, fmap_rs, fmap_gs = m(y, yh)
            for h in hooks:
                h.remove()
            l_disc, _, _ = loss_mod.discriminator_loss(y_d_rs, y_d_gs)
            l_feat = loss_mod.feature_loss(fmap_rs, fmap_gs)
            l_gen, _ = loss_mod.generator_loss(y_d_gs)
            (l_disc + l_feat + l_gen).backward()
            signs = [o.numpy() > 0 for o in pre0]
            for fr, fg in zip(fmap_rs, fmap_gs):
                signs += [f.detach().numpy() > 0 for f in fr[:-1]] + [f.detach().numpy() > 0 for f in fg[:-1]]
                signs += [(a.detach() - b.detach()).numpy() > 0 for a, b in zip(fr, fg)]
            fm = [[torch.cat([a, b]).detach().numpy() for a, b in zip(fr, fg)] for fr, fg in zip(fmap_rs, fmap_gs)]
            runs[tag] = dict(losses=[float(l_disc), float(l_feat), float(l_gen)], grads={n: q.grad.numpy() for n, q in m.named_parameters()},
                             dyh=yh.grad.numpy(), fm=fm, signs=signs)
        flips = sum(int((a != b).sum()) for a, b in zip(runs["32"]["signs"], runs["64"]["signs"]))
        print("train_step seed", seed, "sign flips fp32 vs float64:", flips, "of", sum(a.size for a in runs["64"]["signs"]))
        if flips == 0:
            chosen = seed
            break
    assert chosen is not None, "no seed of TRAIN_STEP['seeds'] is free of sign flips"
    r64, r32 = runs["64"], runs["32"]
    assert all(np.array_equal(a, b) for a, b in zip(r32["signs"], r64["signs"]))
    names = list(sd)
    assert names == list(r64["grads"])
    assert len(names) == 234 and sum(v.size for v in sd.values()) == 1413990
    assert list(m.state_dict()) == list(R.with_windows(sd)) and len(m.state_dict()) == 237
    case = "train_step"
    res[f"{case}/seed"] = np.int64(chosen)
    res[f"{case}/names"] = np.array(names)
    res[f"{case}/shapes"] = np.array([",".join(map(str, sd[n].shape)) for n in names])
    res[f"{case}/state_names"] = np.array(list(m.state_dict()))          # 234 parameters and the three spec_fn.window buffers
    res[f"{case}/state_shapes"] = np.array([",".join(map(str, v.shape)) for v in m.state_dict().values()])
    res[f"{case}/losses64"] = np.array(r64["losses"])
    res[f"{case}/losses32"] = np.array(r32["losses"])
    err = []
    for i, n in enumerate(names):
        res[f"{case}/grad/{n}"] = R.stored(i, r64["grads"][n], chosen)
        err.append(R.rel_l2(R.stored(i, r32["grads"][n], chosen), res[f"{case}/grad/{n}"]))
    res[f"{case}/err32"] = np.array(err)
    res[f"{case}/dyhat64"] = r64["dyh"]
    res[f"{case}/dyhat_err32"] = np.float64(R.rel_l2(r32["dyh"], r64["dyh"]))
    ferr = []
    for k in range(len(R.FFT_SIZES)):
        for i in range(21):
            key = 2000 + 100 * k + i
            res[f"{case}/fmap/{k}/{i}"] = R.stored(key, r64["fm"][k][i], chosen)
            ferr.append(R.rel_l2(R.stored(key, r32["fm"][k][i], chosen), res[f"{case}/fmap/{k}/{i}"]))
        res[f"{case}/logits/{k}"] = r64["fm"][k][20]
    res[f"{case}/fmap_err32"] = np.array(ferr).reshape(len(R.FFT_SIZES), 21)
    print(case, "fp32 vs float64: losses", r32["losses"], r64["losses"], "grad max", max(err), "min", min(err), "dyhat", float(res[f"{case}/dyhat_err32"]),
          "fmaps max", max(ferr), "min", min(ferr))
    _save(OUT, res)
    first = hashlib.sha256(open(OUT, "rb").read()).hexdigest()
    _save(OUT, res)
    assert hashlib.sha256(open(OUT, "rb").read()).hexdigest() == first
    print("wrote", OUT, os.path.getsize(OUT), "bytes, sha256", first)
    assert os.path.getsize(OUT) < 1000 * 1000


if __name__ == "__main__":
    main()
