"""Generates tests/golden/vocos_grads.npz and vocos_grads_frames.npz: gradients of the REAL reference Vocos generator (vocoders/vocos/models/model.py,
unmodified, CPU, one thread) under torch autograd, for the native training path (stabletts_amd/vocos_train.py).  Run where a
checkout of the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_vocos_grads.py

Weights: oracle.vocos_oracle.make_vocos_state_dict(seed); mels: make_mel.  Cases (tests/vocos_vjp_restatement.CASES): the preset
at B = 2, T = 40 and a small config at B = 3, T = 7 with loss = sum(audio * W), W seeded (loss_weights); the preset with the
real MultiScaleMelSpectrogramLoss(y, Vocos(mel).unsqueeze(1)) of vocoders/vocos/train.py:115, y from
tests/golden/mel_loss_grads.npz (B = 2 x 8192 samples -> T = 16), the loss module loaded as tools/make_golden_mel_loss.py loads it.

Every case runs twice, the module in fp32 and in float64 (.double()).  Stored per case from the float64 run: loss64, the sorted
parameter names, per parameter the gradient norm and max |g|, the gradient itself (whole up to FULL_MAX elements, else 512 fixed
sampled elements: vocos_vjp_restatement.stored_elements) and d mel whole.  From the fp32 run: loss32 and, per parameter and for
d mel, err32 = the relative L2 distance of its stored elements from the float64 ones -- the yardstick of the GPU test; the fp32
gradients themselves are not kept (with them, or with whole tensors up to 4096 elements, the file passes 1 MB).
The generator asserts that no exp(a) reaches the head's clip at 100 in any case.  Fixed zip timestamps: regenerating the file
reproduces it byte for byte.

A second table (vocos_vjp_restatement.FRAME_CASES: the small config at 25 x 44 and the preset at 4 x 65 frames, where the split-K
weight gradients of the native path take several planes) goes to tests/golden/vocos_grads_frames.npz with the same keys.  Two
differences: d mel is stored as 4096 sampled elements (vocos_vjp_restatement.sampled; whole it would be 563 KB at 25 x 64 x 44)
and so is the audio (audio64, audio_err32), and the clip IS reached at 25 x 44, so the generator asserts instead that no
log-magnitude lies within 1e-4 of ln 100, in either precision.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "vocos_grads.npz")
OUT_FRAMES = os.path.join(ROOT, "tests", "golden", "vocos_grads_frames.npz")


def _rel_l2(a, ref):
    return float(np.linalg.norm(a.astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref_dir, "vocoders", "vocos", "models", "model.py")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ref_dir)
    torch.set_num_threads(1)
    from make_golden_mel import _install_torchaudio_standin, _save
    _install_torchaudio_standin()
    from config import MelConfig, VocosConfig
    from vocoders.vocos.models.model import Vocos                     # reference, unmodified
    spec = importlib.util.spec_from_file_location("vocos_loss", os.path.join(ref_dir, "vocoders", "vocos", "models", "loss.py"))
    loss_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(loss_mod)                                 # reference, unmodified
    from tests import vocos_vjp_restatement as R
    y_np = np.load(os.path.join(ROOT, "tests", "golden", "mel_loss_grads.npz"))["y"]

    for out, cases, frames in ((OUT, R.CASES, False), (OUT_FRAMES, R.FRAME_CASES, True)):
        res = _run_cases(cases, frames, Vocos, VocosConfig, MelConfig, loss_mod, y_np)
        _save(out, res)
        print("wrote", out, os.path.getsize(out), "bytes")
        assert os.path.getsize(out) < 1000 * 1000


def _run_cases(cases, frames, Vocos, VocosConfig, MelConfig, loss_mod, y_np):
    """frames: the cases of vocos_grads_frames.npz -- the clip may be reached but not within 1e-4 of it, d mel and the audio are
    stored as sampled elements."""
    from oracle import vocos_oracle as vo
    from tests import vocos_vjp_restatement as R
    res = {}
    for case, (fields, B, T, wseed, mseed, loss_kind) in cases.items():
        cfg = vo.vocos_config(**fields)
        sd = vo.make_vocos_state_dict(wseed, cfg)
        mel_np = vo.make_mel(B, T, mseed, M=cfg.input_channels)
        runs = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            voc = Vocos(VocosConfig(cfg.input_channels, cfg.dim, cfg.intermediate_dim, cfg.num_layers), MelConfig())
            voc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            voc = voc.to(dt)
            peak, near = [], []

            def watch(m, i, o):
                a = o[..., :o.shape[-1] // 2].detach()
                peak.append(float(a.max()))
                near.append(float((a - np.log(100.0)).abs().min()))

            hook = voc.head.out.register_forward_hook(watch)
            mel = torch.from_numpy(mel_np).to(dt).requires_grad_(True)
            audio = voc(mel)
            hook.remove()
            if frames:      # the two precisions must take the same branch of the clip everywhere
                assert near[0] > 1e-4, f"{case}: a log-magnitude lies {near[0]:.1e} from the clip"
            else:
                assert np.exp(peak[0]) < 100.0, f"{case}: exp(a) reaches the clip ({np.exp(peak[0]):.1f})"
            if loss_kind == "linear":
                loss = (audio * torch.from_numpy(R.loss_weights(tuple(audio.shape), wseed)).to(dt)).sum()
            else:
                assert tuple(audio.shape) == (y_np.shape[0], y_np.shape[2])
                loss = loss_mod.MultiScaleMelSpectrogramLoss().to(dt)(torch.from_numpy(y_np).to(dt), audio.unsqueeze(1))
            loss.backward()
            grads = {n: p.grad.numpy() for n, p in voc.named_parameters()}
            runs[tag] = (float(loss.item()), grads, mel.grad.numpy(), audio.detach().numpy())
            print(case, tag, "loss", loss.item(), "max a", peak[0], "nearest to the clip", near[0])
        l64, g64, dm64, au64 = runs["64"]
        l32, g32, dm32, au32 = runs["32"]
        names = sorted(g64)
        assert names == R.param_names(sd)
        res[f"{case}/names"] = np.array(names)
        res[f"{case}/loss64"] = np.float64(l64)
        res[f"{case}/loss32"] = np.float64(l32)
        res[f"{case}/norms"] = np.array([float(np.linalg.norm(g64[n])) for n in names])
        res[f"{case}/absmax"] = np.array([float(np.abs(g64[n]).max()) for n in names])
        err = []
        for i, n in enumerate(names):
            ref = R.stored_elements(i, g64[n], wseed)
            res[f"{case}/grad/{n}"] = ref
            err.append(_rel_l2(R.stored_elements(i, g32[n], wseed), ref))
        res[f"{case}/err32"] = np.array(err)
        if frames:
            dm64, dm32 = R.sampled(dm64, wseed, 0), R.sampled(dm32, wseed, 0)
            res[f"{case}/audio64"] = R.sampled(au64, wseed, 1)
            res[f"{case}/audio_err32"] = np.float64(_rel_l2(R.sampled(au32, wseed, 1), res[f"{case}/audio64"]))
        res[f"{case}/dmel64"] = dm64
        res[f"{case}/dmel_err32"] = np.float64(_rel_l2(dm32, dm64))
        print(case, "fp32 vs float64: loss", abs(l32 - l64) / abs(l64), "grad rel L2 max", max(err), "median", float(np.median(err)),
              "dmel", float(res[f"{case}/dmel_err32"]))
    return res


if __name__ == "__main__":
    main()
