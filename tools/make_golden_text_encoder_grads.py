"""Generates tests/golden/text_encoder_grads.npz: gradients of the REAL reference TextEncoder (models/text_encoder.py,
unmodified; fp32, CPU, eval mode so dropout is off) with the seeded weights of oracle.make_text_encoder_state_dict(2468)
(non-zero adaLN: with the adaLN-Zero init every block gradient except adaLN's would be zero).  Run where a checkout of the
reference StableTTS is available:

    STABLETTS_REFERENCE=<path to StableTTS> python tools/make_golden_text_encoder_grads.py

Loss = sum(mu_x * W_mu) + sum(x * W_x) with seeded random projections (loss_weights below), so both the d mu_x and the d x paths
of the backward are exercised.  Per case it stores the loss, d c, the norm of every parameter gradient, in full the gradients of
proj.* (proj.weight in the small case only), of encoder.1.adaLN_modulation.2.bias and the emb.weight rows of the tokens that occur (<case>/emb_ids), and the inputs
(oracle.make_golden_text_encoder.text_inputs).  Cases:
  small  B=3, T=37, lengths [37, 25, 9]
  edge   B=2, T=70, lengths [1, 64]: a length-1 item, an all-padded tail, a 64-frame tile edge
The npz is written with fixed zip timestamps, so regenerating it reproduces the committed file byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "text_encoder_grads.npz")
CASES = {"small": (3, 37, [37, 25, 9], 31), "edge": (2, 70, [1, 64], 32)}
FULL = ("proj.weight", "proj.bias", "encoder.1.adaLN_modulation.2.bias")


def loss_weights(B, T, seed, out_channels=128, hidden=256):
    """The seeded projections of the loss: W_mu (B, out, T), W_x (B, hidden, T)."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    w_mu = rng.standard_normal((B, out_channels, T)).astype(np.float32)
    w_x = (rng.standard_normal((B, hidden, T)) * 0.1).astype(np.float32)
    return torch.from_numpy(w_mu), torch.from_numpy(w_x)


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    ref_dir = os.environ.get("STABLETTS_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref_dir, "models", "text_encoder.py")):
        raise SystemExit("set STABLETTS_REFERENCE to a checkout of the reference StableTTS")
    sys.path.insert(0, ref_dir)
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    from models.text_encoder import TextEncoder               # reference, unmodified
    from oracle.make_golden_text_encoder import text_inputs
    from oracle.weights import TextEncoderConfig, make_text_encoder_state_dict
    cfg = TextEncoderConfig()
    enc = TextEncoder(cfg.n_vocab, cfg.out_channels, cfg.hidden_channels, cfg.filter_channels, cfg.n_heads,
                      cfg.n_layers, cfg.kernel_size, cfg.p_dropout, cfg.gin_channels).eval()
    enc.load_state_dict(make_text_encoder_state_dict(2468, cfg), strict=True)
    res = {}
    for case, (B, T, lengths, seed) in CASES.items():
        tok, c, lens = text_inputs(B, T, lengths, seed)
        w_mu, w_x = loss_weights(B, T, seed)
        enc.zero_grad()
        c = c.clone().requires_grad_(True)
        x, mu_x, _ = enc(tok, c, lens)
        loss = (mu_x * w_mu).sum() + (x * w_x).sum()
        loss.backward()
        res[f"{case}/tokens"], res[f"{case}/c"], res[f"{case}/lengths"] = tok.numpy(), c.detach().numpy(), lens.numpy()
        res[f"{case}/loss"] = np.float64(loss.item())
        res[f"{case}/grad_c"] = c.grad.numpy()
        grads = {n: p.grad for n, p in enc.named_parameters()}
        res[f"{case}/norm_names"] = np.array(sorted(grads))
        res[f"{case}/norms"] = np.array([float(grads[n].double().norm()) for n in sorted(grads)])
        for n in FULL:
            if n != "proj.weight" or case == "small":      # (proj.weight in full once: 128 KB of incompressible floats per case)
                res[f"{case}/full/{n}"] = grads[n].numpy()
        ids = np.unique(np.concatenate([tok[b, :lengths[b]].numpy() for b in range(B)]))
        res[f"{case}/emb_ids"] = ids
        res[f"{case}/emb_rows"] = grads["emb.weight"][torch.from_numpy(ids)].numpy()
        print(case, "loss", loss.item(), "|d c|", float(c.grad.norm()), len(ids), "token rows")
    _save(OUT, res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
