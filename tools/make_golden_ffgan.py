"""Generates tests/golden/ffgan_outputs.npz: outputs of the REAL reference FireflyGANBase (vocoders/ffgan/model.py, unmodified,
``.double()``, CPU) for the native vocoder (stabletts_amd/ffgan.py).  Run where a checkout of the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_ffgan.py

Weights and mels: tests/ffgan_restatement.py (SEED, MEL_SEED, CASES: make_state_dict(DEFAULT, SEED), make_mel(B, T, 128, MEL_SEED + case index)).  Stored:

  state_names / state_shapes        the reference module's state_dict, in its order
  <B>x<T>/audio, encoder, pre_tanh  float64 outputs of the reference module: the audio (B, T * 512), the ConvNeXtEncoder output
                                    (B, 512, T) and the input of the final tanh (B, T * 512), the last two through forward hooks
  <B>x<T>/emul_<dtype>              for dtype in f16, bf16: 3 x 3 floats, rows = (weights and inputs, weights only, inputs only) rounded
                                    to the dtype in the float64 restatement (tests/ffgan_restatement.py: where the native kernels round),
                                    columns = max |emulated - float64| / max |float64| of (audio, encoder, pre_tanh)

The tool asserts that the restatement reproduces the reference module to 1e-10, that the seeded weights keep the signal alive (for
every case with T >= 13, where conv_pre's 13 taps see real frames: every level's std in [0.1, 10], the pre-tanh std in [0.2, 1.5]),
and prints the emulation table (the split by weights / inputs is what a later hi + lo decision needs).

It also writes tests/golden/ffgan_config_outputs.npz: the reference's own ``ConvNeXtEncoder(**cfg["backbone"])`` and
``HiFiGANGenerator(**cfg["head"])`` in float64, composed as FireflyGANBase.forward composes them, at the two non-default
configurations of tests/ffgan_restatement.py: REF_CASES (make_state_dict(cfg, SEED), make_mel(B, T, mels, mel seed)).  Stored per case:
``<name>/audio, encoder, pre_tanh`` and ``<name>/emul_<dtype>`` as above; the restatement is asserted to match to 1e-10 here too.

Fixed zip timestamps: regenerating the files reproduces them byte for byte.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ffgan_outputs.npz")
OUT_CONFIGS = os.path.join(ROOT, "tests", "golden", "ffgan_config_outputs.npz")


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE")
    if not ref_dir or not os.path.isfile(os.path.join(ref_dir, "vocoders", "ffgan", "model.py")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ref_dir)
    torch.manual_seed(0)
    from make_golden_mel import _save
    from tests import ffgan_restatement as R
    from vocoders.ffgan.model import FireflyGANBase      # reference, unmodified

    model = FireflyGANBase().double().eval()
    ref_sd = model.state_dict()
    arrays = {"state_names": np.array(list(ref_sd)), "state_shapes": np.array([";".join(map(str, v.shape)) for v in ref_sd.values()])}
    sd = R.make_state_dict(R.DEFAULT, R.SEED)
    model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    taps = {}
    model.backbone.register_forward_hook(lambda m, i, o: taps.__setitem__("encoder", o.detach().clone()))
    model.head.conv_post.register_forward_hook(lambda m, i, o: taps.__setitem__("pre_tanh", o.detach().clone().squeeze(1)))
    for ci, (B, T) in enumerate(R.CASES):
        mel = R.make_mel(B, T, 128, R.MEL_SEED + ci)
        with torch.no_grad():
            audio = model(mel.double())
        mine = R.forward(sd, R.DEFAULT, mel)
        for name, ref in (("audio", audio), ("encoder", taps["encoder"]), ("pre_tanh", taps["pre_tanh"])):
            err = R.rel_max(mine[name], ref)
            assert err < 1e-10, (B, T, name, err)
            arrays[f"{B}x{T}/{name}"] = ref.numpy()
        stds = [float(l.std()) for l in mine["levels"]]
        pre_std = float(mine["pre_tanh"].std())
        print(f"case {B}x{T}: level std {['%.3f' % s for s in stds]}, pre-tanh std {pre_std:.3f}, max |audio| {float(audio.abs().max()):.3f}")
        if T >= 13:
            assert all(0.1 <= s <= 10 for s in stds) and 0.2 <= pre_std <= 1.5, (stds, pre_std)
        for dt in ("f16", "bf16"):
            rows = []
            for rw, rx in ((dt, dt), (dt, None), (None, dt)):
                em = R.forward(sd, R.DEFAULT, mel, rw, rx)
                rows.append([R.rel_max(em[n], mine[n]) for n in ("audio", "encoder", "pre_tanh")])
            arrays[f"{B}x{T}/emul_{dt}"] = np.array(rows)
            for label, r in zip(("weights+inputs", "weights only", "inputs only"), rows):
                print(f"  {dt:>4} {label:<15} audio {r[0]:.3e}  encoder {r[1]:.3e}  pre_tanh {r[2]:.3e}")
    _save(OUT, arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} kB)")

    # ---- tests/golden/ffgan_config_outputs.npz: the reference's own encoder and head at the configurations of R.REF_CASES
    from vocoders.ffgan.backbone import ConvNeXtEncoder      # reference, unmodified
    from vocoders.ffgan.head import HiFiGANGenerator

    class Composed(torch.nn.Module):      # FireflyGANBase (model.py:44-57) with the configuration as an argument
        def __init__(self, cfg):
            super().__init__()
            self.backbone = ConvNeXtEncoder(**cfg["backbone"])
            self.head = HiFiGANGenerator(**cfg["head"])
            self.head.checkpointing = False

        def forward(self, x):
            return self.head(self.backbone(x)).squeeze(1)

    arrays = {}
    for name, (cfg, B, T, mel_seed) in R.REF_CASES.items():
        model = Composed(cfg).double().eval()
        sd = R.make_state_dict(cfg, R.SEED)
        assert list(model.state_dict()) == list(sd), name      # make_state_dict's name order is the modules'
        model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        taps = {}
        model.backbone.register_forward_hook(lambda m, i, o: taps.__setitem__("encoder", o.detach().clone()))
        model.head.conv_post.register_forward_hook(lambda m, i, o: taps.__setitem__("pre_tanh", o.detach().clone().squeeze(1)))
        mel = R.make_mel(B, T, cfg["backbone"]["input_channels"], mel_seed)
        with torch.no_grad():
            audio = model(mel.double())
        mine = R.forward(sd, cfg, mel)
        for tensor, ref in (("audio", audio), ("encoder", taps["encoder"]), ("pre_tanh", taps["pre_tanh"])):
            err = R.rel_max(mine[tensor], ref)
            assert err < 1e-10, (name, tensor, err)
            arrays[f"{name}/{tensor}"] = ref.numpy()
        stds = [float(l.std()) for l in mine["levels"]]
        pre_std = float(mine["pre_tanh"].std())
        print(f"case {name} {B}x{T}: level std {['%.3f' % s for s in stds]}, pre-tanh std {pre_std:.3f}, max |audio| {float(audio.abs().max()):.3f}")
        for dt in ("f16", "bf16"):
            rows = []
            for rw, rx in ((dt, dt), (dt, None), (None, dt)):
                em = R.forward(sd, cfg, mel, rw, rx)
                rows.append([R.rel_max(em[n], mine[n]) for n in ("audio", "encoder", "pre_tanh")])
            arrays[f"{name}/emul_{dt}"] = np.array(rows)
            assert all(e < 2e-2 for e in rows[0]), (name, dt, rows[0])      # the condition of the GPU gate on its input
            for label, r in zip(("weights+inputs", "weights only", "inputs only"), rows):
                print(f"  {dt:>4} {label:<15} audio {r[0]:.3e}  encoder {r[1]:.3e}  pre_tanh {r[2]:.3e}")
    _save(OUT_CONFIGS, arrays)
    print(f"wrote {OUT_CONFIGS} ({os.path.getsize(OUT_CONFIGS) / 1e3:.0f} kB)")


if __name__ == "__main__":
    main()
