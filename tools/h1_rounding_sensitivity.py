#!/usr/bin/env python
"""Companion of tools/qk_rounding_sensitivity.py (CPU, fp32 oracle only): how much of the one-evaluation error in the arg-max regime is carried by
the 16-bit rounding of the q/k/v projections' INPUT h1 (the LayerNorm output), which hi + lo pairs of q, k, v cannot remove?  B = 2 x T = 1000
ragged, trained-like gates (ada_std 0.15), q/k weights x3 and x1.  Round 6 result (x3): h1 -> f16 for q, k only 1.85e-3 (more than q, k's own rounding,
1.5e-3), for v only 5.3e-4; h1 + q, k, v all rounded 2.5e-3; h1 + v rounded with q, k exact (= attention_precision="split" as built) 1.9e-3 -- which is
why the split mode moved the native 3.9e-3 only to 3.0e-3.  What would close it is what the TRAINING forward now does for v (ST_TRAIN_VLO): feed the
projection h1 as a hi + lo pair.  Not built for inference.  The last two figures ask what would be left after it: h1 as a pair, q, k split,
v -> f16, with the attention output ao (the out-projection's operand) rounded to f16 and with ao exact -- the difference is what a hi + lo pair
of ao could still remove.  Result (x3): 1.08e-3 with ao -> f16, 5.7e-4 with ao exact: ao's rounding carries 47 % of the remainder, so a build of
the mode has to carry ao as a pair as well (profiles/attn_split_input_parity.txt).
    python tools/h1_rounding_sensitivity.py"""
import os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle
import oracle.estimator_oracle as eo
from oracle.inputs import make_inputs
torch.set_num_threads(min(16, os.cpu_count() or 1))
r16 = lambda x: x.half().float()
pair = lambda x: r16(x) + r16(x - r16(x))      # hi + lo operand pair
inp = make_inputs(2, 1000, seed=81, lengths=[1000, 655])
t = torch.tensor(0.5)
orig = eo.mha
def mha_h1(which, h1=r16, ao=None):
    def mha(sd_, prefix, x, mask, n_heads=4, taps=None, drop=None, subst=None):
        xr = h1(x)
        xq = xr if "qk" in which else x
        xv = xr if "v" in which else x
        q = F.conv1d(xq, sd_[prefix + "conv_q.weight"], sd_[prefix + "conv_q.bias"])
        k = F.conv1d(xq, sd_[prefix + "conv_k.weight"], sd_[prefix + "conv_k.bias"])
        v = F.conv1d(xv, sd_[prefix + "conv_v.weight"], sd_[prefix + "conv_v.bias"])
        a, _ = eo.attention(q, k, v, mask, n_heads, drop, subst)
        if ao is not None:
            a = ao(a)
        return F.conv1d(a, sd_[prefix + "conv_o.weight"], sd_[prefix + "conv_o.bias"])
    return mha
for ada, qk in [(0.15, 3.0), (0.15, 1.0)]:
    sd = oracle.make_state_dict(1234, ada_std=ada)
    for i in range(6):
        for nm in ("q", "k"):
            sd[f"blocks.{i}.block.attn.conv_{nm}.weight"] = sd[f"blocks.{i}.block.attn.conv_{nm}.weight"] * qk
    with torch.inference_mode():
        ref = oracle.decoder_forward(sd, t, inp["z"], inp["mask"], inp["mu"], inp["c"])
        row=[f"ada {ada} qk x{qk}:"]
        for name, which in [("h1->f16 for q,k only", ("qk",)), ("h1->f16 for v only", ("v",)), ("h1->f16 for q,k,v", ("qk","v"))]:
            eo.mha = mha_h1(which)
            try:
                out = oracle.decoder_forward(sd, t, inp["z"], inp["mask"], inp["mu"], inp["c"])
            finally:
                eo.mha = orig
            row.append(f"{name}: {float((out - ref).abs().max() / ref.abs().max()):.2e}")
        # h1 rounded AND q,k,v rounded (the native default) ; h1 rounded + q,k exact (split mode today)
        for name, f in [("h1 + q,k,v -> f16", lambda q, k, v: dict(q=r16(q), k=r16(k), v=r16(v))), ("h1 + v -> f16, q,k split", lambda q, k, v: dict(q=q, k=k, v=r16(v)))]:
            eo.mha = mha_h1(("qk","v"))
            try:
                out = oracle.decoder_forward(sd, t, inp["z"], inp["mask"], inp["mu"], inp["c"], qkv_subst=[f] * 6)
            finally:
                eo.mha = orig
            row.append(f"{name}: {float((out - ref).abs().max() / ref.abs().max()):.2e}")
        # the proposed mode: h1 as a pair, q, k split, v -> f16; the attention output rounded to f16 or left exact
        split_v16 = lambda q, k, v: dict(q=q, k=k, v=r16(v))
        for name, ao in [("h1 pair + q,k split, ao -> f16", r16), ("h1 pair + q,k split, ao exact", None)]:
            eo.mha = mha_h1(("qk","v"), h1=pair, ao=ao)
            try:
                out = oracle.decoder_forward(sd, t, inp["z"], inp["mask"], inp["mu"], inp["c"], qkv_subst=[split_v16] * 6)
            finally:
                eo.mha = orig
            row.append(f"{name}: {float((out - ref).abs().max() / ref.abs().max()):.2e}")
    print("  ".join(row), flush=True)
