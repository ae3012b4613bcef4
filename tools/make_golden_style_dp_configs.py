"""Generates tests/golden/style_dp_configs.npz: outputs and parameter gradients of the REAL reference MelStyleEncoder and
DurationPredictor (models/reference_encoder.py, models/duration_predictor.py, unmodified; fp32, CPU, eval mode so dropout is
off) at the configurations, lengths and masks of tests/synth_weights.STYLE_ALL_CASES / DP_ALL_CASES, with that file's seeded
weights.  Run where a checkout of the reference is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_style_dp_configs.py [--search]

Loss = sum(c * W) resp. sum(logw * W) with seeded random projections (tests/style_dp_restatement.loss_weights).  Per case it
stores the output, the loss and style_dp_restatement.grad_digest of the gradients: per parameter (sorted names) the norm and
max |grad|, every gradient of at most 4096 elements whole and 512 fixed elements of each larger one.

ReLU kinks: a DurationPredictor case with realistic weights is only a fair test if no ReLU pre-activation of a valid token is so
close to 0 that a different fp32 summation order flips it.  The generator asserts, per such case, min |float64 pre-activation|
>= 32 x max |real fp32 module - float64| over both ReLU sites; --search prints, per case, the first weight seed from the
tabled one that satisfies it (then update synth_weights.DP_CONFIG_CASES).  Large cases use the kink-free weights instead.

The npz is written with fixed zip timestamps, so regenerating it reproduces the committed file byte for byte; it must stay no
larger than the largest fixture that tests/golden held before it (reference_outputs.npz).
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "style_dp_configs.npz")
KINK_FACTOR = 32.0          # what tests/test_style_dp_restatement_cpu.py asserts
SEARCH_FACTOR = 64.0        # what a seed must reach here: the fp32 difference moves a little with the CPU's thread count


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def _store(res, R, case, out, loss, mod, seed):
    d = R.grad_digest({n: p.grad.numpy() for n, p in mod.named_parameters()}, seed)
    res[f"{case}/out"] = out.detach().numpy()
    res[f"{case}/loss"] = np.float64(loss.item())
    for k in ("names", "norms", "absmax", "full", "sample"):
        res[f"{case}/{k}"] = d[k]


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
    search = "--search" in sys.argv
    res = {}
    for case, (cfg, B, T, spec, seed) in sw.STYLE_ALL_CASES.items():
        if search:
            break
        style = MelStyleEncoder(cfg[0], style_hidden=cfg[1], style_vector_dim=cfg[2], style_kernel_size=cfg[3], style_head=cfg[4],
                                dropout=0.25).eval()
        style.load_state_dict(sw.style_config_state_dict(cfg), strict=True)
        y, m = sw.style_config_inputs(case)
        c = style(torch.from_numpy(y), torch.from_numpy(m))
        loss = (c * R.loss_weights(tuple(c.shape), seed)).sum()
        loss.backward()
        _store(res, R, case, c, loss, style, seed)
        print(case, "loss", loss.item())
    for case, (cfg, B, T, lengths, seed, wseed) in sw.DP_ALL_CASES.items():
        kink_free = sw.dp_kink_free(cfg, lengths)
        x, m, g = (torch.from_numpy(a) for a in sw.dp_inputs(B, T, lengths, seed, hidden=cfg[0], gin=cfg[3]))
        dp = DurationPredictor(cfg[0], cfg[1], cfg[2], 0.5, cfg[3]).eval()
        pre32 = []
        hooks = [mod.register_forward_hook(lambda _m, _i, o: pre32.append(o.detach())) for mod in (dp.conv1, dp.conv2)]
        for ws in range(wseed, wseed + (5000 if search and not kink_free else 1)):
            sd = sw.duration_predictor_state_dict(ws, hidden=cfg[0], filt=cfg[1], kernel=cfg[2], gin=cfg[3], kink_free=kink_free)
            dp.load_state_dict(sd, strict=True)
            dp.zero_grad()
            del pre32[:]
            logw = dp(x, m, g)
            with torch.no_grad():
                _, pre64 = R.dp_forward({k: v.double() for k, v in sd.items()}, x.double(), m.double(), g.double(), return_pre=True)
            lo, diff = R.kink_margin(pre64, pre32, m)
            if lo >= (KINK_FACTOR if kink_free else SEARCH_FACTOR) * diff:
                break
        else:
            raise SystemExit(f"{case}: no weight seed keeps the ReLU pre-activations {KINK_FACTOR} x the fp32 error from 0")
        print(case, "kink-free" if kink_free else "realistic", "weight seed", ws, f"min |pre| {lo:.3e}, fp32 vs float64 {diff:.3e}")
        assert search or ws == wseed, (case, "run with --search and update synth_weights.DP_CONFIG_CASES")
        for h in hooks:
            h.remove()
        loss = (logw * R.loss_weights(tuple(logw.shape), seed)).sum()
        loss.backward()
        _store(res, R, case, logw, loss, dp, seed)
    if search:
        return
    _save(OUT, res)
    size = os.path.getsize(OUT)
    limit = max(os.path.getsize(os.path.join(os.path.dirname(OUT), f)) for f in os.listdir(os.path.dirname(OUT)) if f != os.path.basename(OUT))
    print("wrote", OUT, size, "bytes; the largest other fixture has", limit)
    assert size <= limit


if __name__ == "__main__":
    main()
