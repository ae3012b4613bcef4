"""Generates tests/golden/vocos_dims.npz: the REAL reference Vocos generator (vocoders/vocos/models/model.py, unmodified, CPU, one
thread) at backbone widths 768 and 1024 and at the configuration the reference's Vocos trainer builds
(vocoders/vocos/config.py:21-26: 128 / 768 / 2048 / 12), forward and torch autograd, in the manner of
tools/make_golden_vocos_grads.py.  Run where a checkout of the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_vocos_dims.py

Cases: tests/vocos_dims_cases.CASES (d768 and d1024: M 64, F 256, 2 layers, B = 3, T = 7; trainer: B = 1, T = 4), weights
make_vocos_state_dict(seed, cfg), mel make_mel, loss = sum(audio * W), W = vocos_vjp_restatement.loss_weights.

Every case runs twice, the module in fp32 and in float64.  Stored per case from the float64 run: loss64, the sorted parameter
names, per parameter the gradient norm, the gradient's stored elements (vocos_dims_cases.stored_elements: whole up to KEEP[case]
elements, else that many fixed sampled ones), d mel whole, the audio as up to 4096 sampled elements (vocos_vjp_restatement.sampled;
the trainer's 2048 samples whole).  From the fp32 run: loss32 and, per parameter, for d mel and for the audio, err32 = the relative
L2 distance of its stored elements from the float64 ones -- the yardstick of the GPU test.  The generator asserts that no
log-magnitude lies within 1e-4 of the head's clip at ln 100, in either precision.  Fixed zip timestamps: regenerating the file
reproduces it byte for byte.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "vocos_dims.npz")


def _rel_l2(a, ref):
    return float(np.linalg.norm(a.astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE", "")
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
    from oracle import vocos_oracle as vo
    from tests import vocos_dims_cases as D
    from tests import vocos_vjp_restatement as R

    res = {}
    for case, (fields, B, T, wseed, mseed, _) in D.CASES.items():
        cfg = vo.vocos_config(**fields)
        sd = vo.make_vocos_state_dict(wseed, cfg)
        mel_np = vo.make_mel(B, T, mseed, M=cfg.input_channels)
        runs = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            voc = Vocos(VocosConfig(cfg.input_channels, cfg.dim, cfg.intermediate_dim, cfg.num_layers), MelConfig())
            voc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            voc = voc.to(dt)
            near = []
            hook = voc.head.out.register_forward_hook(
                lambda m, i, o: near.append(float((o[..., :o.shape[-1] // 2].detach() - np.log(100.0)).abs().min())))
            mel = torch.from_numpy(mel_np).to(dt).requires_grad_(True)
            audio = voc(mel)
            hook.remove()
            assert near[0] > 1e-4, f"{case}: a log-magnitude lies {near[0]:.1e} from the clip"
            loss = (audio * torch.from_numpy(R.loss_weights(tuple(audio.shape), wseed)).to(dt)).sum()
            loss.backward()
            grads = {n: p.grad.numpy() for n, p in voc.named_parameters()}
            runs[tag] = (float(loss.item()), grads, mel.grad.numpy(), audio.detach().numpy())
            print(case, tag, "loss", loss.item(), "nearest to the clip", near[0])
        l64, g64, dm64, au64 = runs["64"]
        l32, g32, dm32, au32 = runs["32"]
        names = sorted(g64)
        assert names == R.param_names(sd)
        res[f"{case}/names"] = np.array(names)
        res[f"{case}/loss64"] = np.float64(l64)
        res[f"{case}/loss32"] = np.float64(l32)
        res[f"{case}/norms"] = np.array([float(np.linalg.norm(g64[n])) for n in names])
        err = []
        for i, n in enumerate(names):
            ref = D.stored_elements(case, i, g64[n], wseed)
            res[f"{case}/grad/{n}"] = ref
            err.append(_rel_l2(D.stored_elements(case, i, g32[n], wseed), ref))
        res[f"{case}/err32"] = np.array(err)
        res[f"{case}/audio64"] = R.sampled(au64, wseed, 1)
        res[f"{case}/audio_err32"] = np.float64(_rel_l2(R.sampled(au32, wseed, 1), res[f"{case}/audio64"]))
        res[f"{case}/dmel64"] = dm64
        res[f"{case}/dmel_err32"] = np.float64(_rel_l2(dm32, dm64))
        print(case, "fp32 vs float64: loss", abs(l32 - l64) / abs(l64), "grad rel L2 max", max(err), "median", float(np.median(err)),
              "audio", float(res[f"{case}/audio_err32"]), "dmel", float(res[f"{case}/dmel_err32"]))
    _save(OUT, res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 400 * 1000


if __name__ == "__main__":
    main()
