"""Generates tests/golden/synthesise_outputs.npz from the REAL reference modules (models/reference_encoder.py,
models/duration_predictor.py and the whole models/model.py StableTTS.synthesise, unmodified) with the seeded weights and
inputs of tests/synth_weights.py.  Run where a checkout of the reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_synthesise.py [--search]

Import stand-ins only for packages absent offline: numba (monotonic_align's decorator, training only) and torchdiffeq
(the fixed-grid stand-in of oracle/make_golden.py).  The decoder's torch.randn_like draw (flow_matching.py:45) is replaced
by the seeded noise z, which the fixture stores.  --search looks for the first DP seed from synth_weights.DP_SEED on whose
durations every valid token clears the ceil() margin; without it the generator asserts that DP_SEED does.
The npz is written with fixed zip timestamps, so regenerating it reproduces the committed file byte for byte.
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "synthesise_outputs.npz")
MODEL_ARGS = (401, 128, 256, 1024, 4, 3, 6, 3, 0.1, 256)       # models/model.py:33 as config.py's ModelConfig sets it


def _install_standins():
    from oracle.make_golden import _install_torchdiffeq_standin

    class _Ty:
        def __getitem__(self, item):
            return self

        def __call__(self, *a, **k):
            return self

    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (lambda f: f)
    numba.void = numba.int32 = numba.float32 = _Ty()
    sys.modules["numba"] = numba
    _install_torchdiffeq_standin()


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def durations(logw, mask, length_scale):
    """models/model.py:83-85."""
    w = torch.exp(logw) * mask
    w_ceil = torch.ceil(w) * length_scale
    y_lengths = torch.clamp_min(torch.sum(w_ceil, [1, 2]), 1).long()
    return w_ceil, y_lengths


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref_dir, "models")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, ref_dir)
    torch.set_num_threads(1)              # CPU reductions in one fixed order: the file regenerates byte for byte
    _install_standins()
    from tests import synth_weights as sw
    from oracle.weights import make_state_dict, make_text_encoder_state_dict
    from models.model import StableTTS     # reference, unmodified (imports the reference encoder / predictor)
    from models.reference_encoder import MelStyleEncoder
    from models.duration_predictor import DurationPredictor
    assert MelStyleEncoder.__module__ == "models.reference_encoder" and DurationPredictor.__module__ == "models.duration_predictor"

    model = StableTTS(*MODEL_ARGS).eval()
    s = sw.SYNTH
    inp = sw.synth_inputs()
    sd = {"encoder." + k: v for k, v in make_text_encoder_state_dict(2468).items()}
    sd.update({"decoder.estimator." + k: v for k, v in make_state_dict(1234).items()})
    sd.update({"ref_encoder." + k: v for k, v in sw.style_encoder_state_dict().items()})
    sd["fake_speaker"] = torch.from_numpy(inp["fake_speaker"])
    sd["fake_content"] = torch.from_numpy(inp["fake_content"])
    tok, lens, y = torch.from_numpy(inp["x"]), torch.from_numpy(inp["x_lengths"]), torch.from_numpy(inp["y"])
    missing, unexpected = model.load_state_dict(sd, strict=False)       # everything but dp.*, which the seed search varies
    assert not unexpected and all(k.startswith("dp.") for k in missing)

    def dp_outputs(seed):
        model.dp.load_state_dict(sw.duration_predictor_state_dict(seed), strict=True)
        res, ok = {}, True
        with torch.inference_mode():
            for name, (B, T, lengths, iseed) in sw.DP_CASES.items():
                x, m, g = (torch.from_numpy(a) for a in sw.dp_inputs(B, T, lengths, iseed))
                logw = model.dp(x, m, g)
                w_ceil, y_len = durations(logw, m, 1.0)
                res[name + "_logw"], res[name + "_w_ceil"], res[name + "_y_lengths"] = logw.numpy(), w_ceil.numpy(), y_len.numpy()
                ok &= sw.clears_margin(logw.numpy(), m.numpy())
            c = model.ref_encoder(y, None)
            x, mu_x, x_mask = model.encoder(tok, c, lens)
            logw = model.dp(x, x_mask, c)
            ok &= sw.clears_margin(logw.numpy(), x_mask.numpy())
        return res, ok

    if "--search" in sys.argv:
        for seed in range(sw.DP_SEED, sw.DP_SEED + 5000):
            if dp_outputs(seed)[1]:
                print("first DP seed clearing the margin:", seed)
                return
        raise SystemExit("no seed found")
    res, ok = dp_outputs(sw.DP_SEED)
    assert ok, "a valid token's duration sits within MARGIN of an integer: run with --search and update DP_SEED"
    sd.update({"dp." + k: v for k, v in sw.duration_predictor_state_dict().items()})
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected

    with torch.inference_mode():
        for name, (B, T, lengths, iseed) in sw.STYLE_CASES.items():
            ym, m = sw.style_inputs(B, T, lengths, iseed)
            res[name + "_c"] = model.ref_encoder(torch.from_numpy(ym), torch.from_numpy(m) if m is not None else None).numpy()
        # the synthesise chain, with its intermediate stages for the tests that chain the native modules
        c = model.ref_encoder(y, None)
        x, mu_x, x_mask = model.encoder(tok, c, lens)
        logw = model.dp(x, x_mask, c)
        w_ceil, y_len = durations(logw, x_mask, s["length_scale"])
        z = torch.from_numpy(sw.synth_noise(s["B"], MODEL_ARGS[1], int(y_len.max())))
        real = torch.randn_like

        def randn_like(t, *a, **k):
            assert t.shape == z.shape, (t.shape, z.shape)
            return z.clone()

        torch.randn_like = randn_like
        try:
            out = model.synthesise(tok, lens, s["n_steps"], 1.0, y, s["length_scale"], s["solver"], s["cfg"])
        finally:
            torch.randn_like = real
    res.update(synth_c=c.numpy(), synth_logw=logw.numpy(), synth_x_mask=x_mask.numpy(), synth_w_ceil=w_ceil.numpy(),
               synth_y_lengths=y_len.numpy(), synth_z=z.numpy(), synth_attn=out["attn"].numpy(),
               synth_encoder_outputs=out["encoder_outputs"].numpy(), synth_decoder_outputs=out["decoder_outputs"].numpy())
    for k in sorted(res):
        print(f"{k:28s} {str(res[k].shape):18s} max|.| {float(np.nanmax(np.abs(res[k]))):.4g}")
    w = np.exp(res["synth_logw"])[res["synth_x_mask"] > 0]
    print("synth w range", w.min(), w.max(), "y_lengths", res["synth_y_lengths"])
    _save(OUT, res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
