"""CPU emulation of where each attention_precision mode rounds the attention branch's operands (test infrastructure).  "16bit" and
"split" are the modes the engine has; "split_input" is the proposed third one, not built.

The fp32 oracle (oracle.decoder_forward) with its multi-head attention replaced by one that rounds h1 (the LayerNorm / modulate output
that feeds the q / k / v projections), q, k, v, the probabilities P and the attention output ao to 16 bits, or to a hi + lo pair of
16-bit values, or not at all.  Everything outside the attention branch stays fp32, so the figures are what THOSE operands carry.
tools/h1_rounding_sensitivity.py makes the same substitutions by hand; tests/test_attn_split_input_cpu.py pins this module against the
figures that tool published.  (The max-norm figure in the arg-max regime moves by ~10 % with the fp32 formulation of the softmax, so
where P is exact the oracle's own torch.softmax is used, as the tool does.)

An operand spec is "exact" (fp32), "f16" (one 16-bit value) or "pair" (hi = fl16(x), lo = fl16(x - hi), used as hi + lo: 22 bits)."""
import math

import torch
import torch.nn.functional as F

import oracle
import oracle.estimator_oracle as eo


def r16(x):
    return x.half().float()


def pair(x):
    hi = r16(x)
    return hi + r16(x - hi)


_ROUND = {"exact": lambda x: x, "f16": r16, "pair": pair}

# where the kernels of each mode round (st_set_option "attention_precision" 0 / 1) or would round ("split_input")
MODES = {
    "16bit": dict(h1_qk="f16", h1_v="f16", qk="f16", v="f16", p="f16", ao="f16"),
    "split": dict(h1_qk="f16", h1_v="f16", qk="pair", v="f16", p="f16", ao="f16"),
    "split_input": dict(h1_qk="pair", h1_v="pair", qk="pair", v="f16", p="f16", ao="pair"),
}


# The two shapes for a GPU test of the mode: A = 2 * 4 * ceil(300 / 256) = 16 attention blocks, the small-grid kernel's range in the
# 16-bit mode; B = 36 blocks, the big kernel in every mode (with split q / k operands launch_attention always takes the big kernel's
# SPLIT form).  Both kept: the emulated gain of "split_input" over "split" in
# the arg-max regime is 74 % (A) and 76 % (B) of the emulated "split" error, far above the 20 % below which a shape would say nothing.
SHAPES = {"A": dict(B=2, T=300, lengths=[300, 211]), "B": dict(B=3, T=520, lengths=[520, 401, 77])}


def shape_inputs(name):
    from oracle.inputs import make_inputs
    sh = SHAPES[name]
    return make_inputs(sh["B"], sh["T"], lengths=sh["lengths"])


def trained_like(ada, qk, n_layers=6):
    """Seeded weights with adaLN gates of std `ada` and the q / k projections scaled by `qk` (test_gpu_parity.py: _trained_like)."""
    sd = oracle.make_state_dict(1234, ada_std=ada)
    for i in range(n_layers):
        for nm in ("q", "k"):
            sd[f"blocks.{i}.block.attn.conv_{nm}.weight"] = sd[f"blocks.{i}.block.attn.conv_{nm}.weight"] * qk
    return sd


def _mha(spec):
    rq, rv = _ROUND[spec.get("h1_qk", "exact")], _ROUND[spec.get("h1_v", "exact")]
    rqk, rvv = _ROUND[spec.get("qk", "exact")], _ROUND[spec.get("v", "exact")]
    rp, rao = _ROUND[spec.get("p", "exact")], _ROUND[spec.get("ao", "exact")]

    def mha(sd, prefix, x, mask, n_heads=4, taps=None, drop=None, subst=None):
        q = F.conv1d(rq(x), sd[prefix + "conv_q.weight"], sd[prefix + "conv_q.bias"])
        k = F.conv1d(rq(x), sd[prefix + "conv_k.weight"], sd[prefix + "conv_k.bias"])
        v = F.conv1d(rv(x), sd[prefix + "conv_v.weight"], sd[prefix + "conv_v.bias"])
        B, C, T = q.shape
        dh = C // n_heads
        qh, kh, vh = (z.view(B, n_heads, dh, T).transpose(2, 3) for z in (q, k, v))
        qh, kh, vh = rqk(eo.rope(qh, dh // 2)), rqk(eo.rope(kh, dh // 2)), rvv(vh)
        am = mask.unsqueeze(1) * mask.unsqueeze(-1)
        am = torch.zeros_like(am).masked_fill(am == 0, -torch.finfo(q.dtype).max)
        s = torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(dh) + am
        if spec.get("p", "exact") == "exact":      # the oracle's own softmax (oracle.estimator_oracle.attention)
            o = torch.matmul(torch.softmax(s, dim=-1), vh)
        else:      # the kernels feed the UNNORMALISED probabilities exp(s - max) to the P V product and divide by their fp32 sum afterwards
            p = torch.exp(s - s.amax(dim=-1, keepdim=True))
            o = torch.matmul(rp(p), vh) / p.sum(dim=-1, keepdim=True)
        a = rao(o.transpose(2, 3).contiguous().view(B, C, T))
        if taps is not None:
            taps["q"], taps["k"], taps["v"], taps["attn"] = qh, kh, vh, a
        return F.conv1d(a, sd[prefix + "conv_o.weight"], sd[prefix + "conv_o.bias"])
    return mha


def forward(sd, t, inp, spec=None, taps=None):
    """One oracle evaluation with the attention branch's operands rounded as `spec` says (None: the plain fp32 oracle)."""
    orig = eo.mha
    if spec is not None:
        eo.mha = _mha(spec)
    try:
        with torch.inference_mode():
            return oracle.decoder_forward(sd, t, inp["z"], inp["mask"], inp["mu"], inp["c"], taps=taps)
    finally:
        eo.mha = orig


def rel(out, ref):
    return float((out.double() - ref.double()).abs().max() / ref.double().abs().max())


def error(sd, t, inp, spec, ref=None):
    """max |emulated - fp32| / max |fp32| of one evaluation."""
    if ref is None:
        ref = forward(sd, t, inp)
    return rel(forward(sd, t, inp, spec), ref)
