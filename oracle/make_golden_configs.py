"""Generates tests/golden/config_outputs.npz: the REAL reference CFMDecoder (/root/reference/models/flow_matching.py,
estimator.py and diffusion_transformer.py, unmodified) at decoder configs other than the default, so that the oracle's
handling of filter_channels, gin_channels and n_layers is pinned before the native engine is compared with it there.
For every case of CASES it stores one estimator evaluation, a 3-step Euler solve with CFG (torchdiffeq stand-in of
make_golden.py), the loss with its random draws, and gradient summaries in the format of loss_grads.npz (every
parameter's gradient norm, a few tensors in full, d mu and d c).  Run where /root/reference is mounted:

    python oracle/make_golden_configs.py
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "config_outputs.npz")

# name: (filter_channels, gin_channels, n_layers, weight seed).  F = 384 and 128 are not multiples of 256, G = 260 is not a
# multiple of 64 and G = 4 is the smallest accepted, L = 2 has one long skip.
CASES = {"f384_g260_l2": (384, 260, 2, 51), "f128_g4_l4": (128, 4, 4, 52)}
B, T, LENGTHS = 2, 40, [40, 27]
FULL = ["final_proj.bias", "in_proj.bias", "blocks.0.block.adaLN_modulation.0.bias", "blocks.0.block.mlp.conv_1.bias",
        "lsc_layers.0.bias", "cond_proj.2.bias"]      # stored in full


def config(name):
    from oracle.weights import DecoderConfig
    f, g, n_layers, _ = CASES[name]
    return DecoderConfig(filter_channels=f, gin_channels=g, n_layers=n_layers)


def state_dict(name):
    from oracle.weights import make_state_dict
    return make_state_dict(CASES[name][3], config(name))


def case_inputs(name, seed_offset=0):
    from oracle.inputs import make_inputs
    return make_inputs(B, T, seed=CASES[name][3] + seed_offset, lengths=LENGTHS, gin=config(name).gin_channels)


def main():
    if not os.path.isdir(REF):
        raise SystemExit(f"reference not mounted at {REF}")
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    from oracle.make_golden import _install_torchdiffeq_standin
    _install_torchdiffeq_standin()
    from models.flow_matching import CFMDecoder               # reference, unmodified
    from oracle.weights import make_cfg_params
    from oracle.inputs import make_inputs

    res = {}
    for name in CASES:
        cfg = config(name)
        dec = CFMDecoder(cfg.noise_channels, cfg.cond_channels, cfg.hidden_channels, cfg.out_channels, cfg.filter_channels,
                         cfg.n_heads, cfg.n_layers, cfg.kernel_size, cfg.p_dropout, cfg.gin_channels).eval()
        dec.estimator.load_state_dict(state_dict(name), strict=True)
        fs, fc = make_cfg_params(CASES[name][3] + 1000, cfg)
        inp = case_inputs(name)
        with torch.no_grad():          # (not inference_mode: the rotary cache it fills is used by the backward below)
            res[name + ".nfe"] = dec.estimator(torch.tensor(0.4), inp["z"], inp["mask"], inp["mu"], inp["c"])
            torch.manual_seed(CASES[name][3])
            z = torch.randn_like(inp["mu"])                   # what flow_matching.py:45 draws (temperature 1)
            torch.manual_seed(CASES[name][3])
            res[name + ".solve"] = dec(inp["mu"], inp["mask"], 3, 1.0, inp["c"], "euler",
                                       dict(fake_speaker=fs, fake_content=fc, cfg_strength=3.0))
            res[name + ".solve_z"] = z

        x1 = make_inputs(B, T, seed=CASES[name][3] + 100)["z"]
        linp = case_inputs(name, 200)
        mu = linp["mu"].clone().requires_grad_(True)
        c = linp["c"].clone().requires_grad_(True)
        torch.manual_seed(7)
        res[name + ".loss_t_rand"] = torch.rand([B, 1, 1])    # the draws of flow_matching.py:75-80
        res[name + ".loss_z"] = torch.randn_like(x1)
        torch.manual_seed(7)
        loss, _ = dec.compute_loss(x1, linp["mask"], mu, c)
        loss.backward()
        res[name + ".loss_value"] = loss.detach().reshape(1)
        res[name + ".grad_mu"], res[name + ".grad_c"] = mu.grad, c.grad
        norms = []
        for pname, p in dec.estimator.named_parameters():
            norms.append(float(p.grad.double().norm()))
            if pname in FULL:
                res[name + ".grad." + pname] = p.grad
        res[name + ".names"] = [pname for pname, _ in dec.estimator.named_parameters()]
        res[name + ".grad_norms"] = torch.tensor(norms, dtype=torch.float64)
        print(name, "loss", float(loss.detach()), "params", len(norms), "|grad| range", min(norms), max(norms))
    out = {k: (np.array(v) if isinstance(v, list) else v.detach().numpy()) for k, v in res.items()}
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
