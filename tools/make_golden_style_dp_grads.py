"""Generates tests/golden/style_dp_grads.npz: parameter gradients of the REAL reference MelStyleEncoder and DurationPredictor
(models/reference_encoder.py, models/duration_predictor.py, unmodified; fp32, CPU, eval mode so dropout is off) with the seeded
weights of tests/synth_weights.py, built as models/model.py:38-39 builds them.  Run where a checkout of the reference is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_style_dp_grads.py

Loss = sum(c * W) resp. sum(logw * W) with seeded random projections (tests/style_dp_restatement.loss_weights).  Per case it
stores the loss, per parameter (sorted names) the gradient norm and max |grad|, the full gradient of every tensor of at most
4096 elements, and 512 fixed elements (style_dp_restatement.sample_index) of each larger one.  The inputs are those of
tests/synth_weights.style_inputs / dp_inputs with the seeds of style_dp_restatement.STYLE_GRAD_CASES / DP_GRAD_CASES.  The
npz is written with fixed zip timestamps, so regenerating it reproduces the committed file byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "style_dp_grads.npz")
FULL_MAX = 4096


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def _grads(res, case, mod, seed):
    grads = {n: p.grad for n, p in mod.named_parameters()}
    names = sorted(grads)
    res[f"{case}/names"] = np.array(names)
    res[f"{case}/norms"] = np.array([float(grads[n].double().norm()) for n in names])
    res[f"{case}/absmax"] = np.array([float(grads[n].abs().max()) for n in names])
    for i, n in enumerate(names):
        g = grads[n].reshape(-1).numpy()
        if g.size <= FULL_MAX:
            res[f"{case}/full/{n}"] = g
        else:
            res[f"{case}/sample/{n}"] = g[__import__("style_dp_restatement").sample_index(g.size, seed + i)]


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref_dir, "models", "reference_encoder.py")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ref_dir)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(1)
    from models.duration_predictor import DurationPredictor       # reference, unmodified
    from models.reference_encoder import MelStyleEncoder
    import style_dp_restatement as R
    import synth_weights as sw
    style = MelStyleEncoder(sw.N_MELS, style_vector_dim=sw.GIN, style_kernel_size=5, dropout=0.25).eval()    # model.py:38
    style.load_state_dict(sw.style_encoder_state_dict(), strict=True)
    dp = DurationPredictor(sw.DP_HIDDEN, sw.DP_FILTER, sw.DP_KERNEL, 0.5, sw.GIN).eval()                     # model.py:39
    dp.load_state_dict(sw.duration_predictor_state_dict(), strict=True)
    res = {}
    for case, (B, T, lengths, seed) in R.STYLE_GRAD_CASES.items():
        y, m = sw.style_inputs(B, T, lengths, seed)
        style.zero_grad()
        c = style(torch.from_numpy(y), torch.from_numpy(m) if m is not None else None)
        loss = (c * R.loss_weights(tuple(c.shape), seed)).sum()
        loss.backward()
        res[f"{case}/loss"] = np.float64(loss.item())
        _grads(res, case, style, seed)
        print(case, "loss", loss.item())
    for case, (B, T, lengths, seed) in R.DP_GRAD_CASES.items():
        x, m, g = sw.dp_inputs(B, T, lengths, seed)
        dp.zero_grad()
        logw = dp(torch.from_numpy(x), torch.from_numpy(m), torch.from_numpy(g))
        loss = (logw * R.loss_weights(tuple(logw.shape), seed)).sum()
        loss.backward()
        res[f"{case}/loss"] = np.float64(loss.item())
        _grads(res, case, dp, seed)
        print(case, "loss", loss.item())
    _save(OUT, res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
