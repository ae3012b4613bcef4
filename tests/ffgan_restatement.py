"""Float64 restatement of the FireflyGAN vocoder (vocoders/ffgan/model.py:44-57, backbone.py:124-214, head.py:101-108,132-133,
226-249 with use_template=False) from a state dict, and the seeded weights and mels of its tests.

``forward(sd, cfg, mel)`` is the reference's arithmetic in float64.  Two switches emulate the native engine's 16-bit MFMA operands:
``round_w`` rounds the weights of every GEMM / convolution that runs on the MFMA, ``round_x`` their inputs, each exactly where the
kernels round (stabletts_amd/csrc/engine_ffgan.cpp):

  encoder   the mel (im2col rows of the stem), every LayerNorm output that feeds a GEMM, the GELU output; the depthwise convs, the
            LayerNorms, the layer scale and the residual stream stay unrounded (fp32 on the device)
  head      the encoder output into conv_pre; silu(x) into every transposed conv and every c1; silu(c1(.) + b) into every c2; the folded
            weight g v / ||v|| of all of them; biases, residual adds, the ParralelBlock mean, SiLU -> conv_post -> tanh stay unrounded

A ResBlock has one conv pair per dilation (the reference always has three).
"""
import numpy as np
import torch
import torch.nn.functional as F

DEFAULT = {
    "backbone": {"input_channels": 128, "depths": [3, 3, 9, 3], "dims": [128, 256, 384, 512], "drop_path_rate": 0.2, "kernel_size": 7},
    "head": {"hop_length": 512, "upsample_rates": [8, 8, 2, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4, 4],
             "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]], "num_mels": 512,
             "upsample_initial_channel": 512, "use_template": False, "pre_conv_kernel_size": 13, "post_conv_kernel_size": 13},
}


def small_config(rates=(4, 2), kernels=(8, 4), rk=(3, 5), rd=((1, 2), (1, 3)), c0=64, pre=7, post=7, depths=(1, 1), dims=(128, 256), mels=64):
    """A supported configuration small enough for float64 on the CPU: every head field differs from the default."""
    hop = int(np.prod(rates))
    return {"backbone": {"input_channels": mels, "depths": list(depths), "dims": list(dims), "drop_path_rate": 0.0, "kernel_size": 7},
            "head": {"hop_length": hop, "upsample_rates": list(rates), "upsample_kernel_sizes": list(kernels),
                     "resblock_kernel_sizes": list(rk), "resblock_dilation_sizes": [list(d) for d in rd], "num_mels": dims[-1],
                     "upsample_initial_channel": c0, "use_template": False, "pre_conv_kernel_size": pre, "post_conv_kernel_size": post}}


# tests/golden/ffgan_outputs.npz (tools/make_golden_ffgan.py): make_state_dict(DEFAULT, SEED), case i = make_mel(B, T, 128, MEL_SEED + i)
SEED, MEL_SEED = 20240, 100
CASES = ((1, 24), (2, 13), (2, 1), (1, 2))

# tests/golden/ffgan_config_outputs.npz (the same tool): the reference's own ConvNeXtEncoder and HiFiGANGenerator at two further
# configurations, name -> (config, B, T, mel seed) with make_state_dict(config, SEED).  Its ResBlock1 always has three dilations.
REF_CASES = {
    "ref_a": (small_config(rates=(6, 10), kernels=(12, 20), rk=(5, 13), rd=((1, 2, 4), (1, 3, 4)), mels=192, dims=(768, 640)), 2, 11, 41),
    "ref_b": (small_config(rates=(16, 2), kernels=(32, 4), rk=(1, 9, 3), rd=((1, 1, 1), (1, 2, 6), (2, 9, 25)), dims=(1024,), depths=(2,),
                           pre=1, post=13), 2, 30, 41),      # head 64 -> 32 -> 16 channels (the last level needs 16)
}

WN0, WN1 ="parametrizations.weight.original0", "parametrizations.weight.original1"


def param_shapes(cfg):
    """[(state_dict name, shape)] in the reference's registration order."""
    b, h = cfg["backbone"], cfg["head"]
    M, dims, depths, K = b["input_channels"], b["dims"], b["depths"], b["kernel_size"]
    out = []
    ds = "backbone.downsample_layers."
    out += [(ds + "0.0.weight", (dims[0], M, K)), (ds + "0.0.bias", (dims[0],)), (ds + "0.1.weight", (dims[0],)), (ds + "0.1.bias", (dims[0],))]
    for i in range(1, len(dims)):
        out += [(ds + f"{i}.0.weight", (dims[i - 1],)), (ds + f"{i}.0.bias", (dims[i - 1],)),
                (ds + f"{i}.1.weight", (dims[i], dims[i - 1], 1)), (ds + f"{i}.1.bias", (dims[i],))]
    for i, C in enumerate(dims):
        for j in range(depths[i]):
            p = f"backbone.stages.{i}.{j}."
            out += [(p + "gamma", (C,)), (p + "dwconv.weight", (C, 1, K)), (p + "dwconv.bias", (C,)), (p + "norm.weight", (C,)), (p + "norm.bias", (C,)),
                    (p + "pwconv1.weight", (4 * C, C)), (p + "pwconv1.bias", (4 * C,)), (p + "pwconv2.weight", (C, 4 * C)), (p + "pwconv2.bias", (C,))]
    out += [("backbone.norm.weight", (dims[-1],)), ("backbone.norm.bias", (dims[-1],))]

    def wn(p, d0, d1, k, nb):
        return [(p + "bias", (nb,)), (p + WN0, (d0, 1, 1)), (p + WN1, (d0, d1, k))]
    C0 = h["upsample_initial_channel"]
    out += wn("head.conv_pre.", C0, h["num_mels"], h["pre_conv_kernel_size"], C0)
    n = len(h["upsample_rates"])
    for i in range(n):
        out += wn(f"head.ups.{i}.", C0 >> i, C0 >> (i + 1), h["upsample_kernel_sizes"][i], C0 >> (i + 1))
    for i in range(n):
        C = C0 >> (i + 1)
        for bi, (k, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            for which in (1, 2):
                for p in range(len(dil)):
                    out += wn(f"head.resblocks.{i}.blocks.{bi}.convs{which}.{p}.", C, C, k, C)
    out += wn("head.conv_post.", 1, C0 >> n, h["post_conv_kernel_size"], 1)
    return out


def make_state_dict(cfg, seed):
    """Seeded weights that keep the signal alive through the whole model (default init leaves max |audio| at 0.03): every level's std
    stays in [0.1, 10] and the pre-tanh std in [0.2, 1.5] (asserted by tools/make_golden_ffgan.py).  The weight-norm gain original0 is
    drawn independently of ||original1||, so a missing fold fails; gamma is of order 0.5, so the ConvNeXt blocks count."""
    rng = np.random.default_rng(seed)
    h = cfg["head"]
    sd = {}
    for name, shape in param_shapes(cfg):
        leaf = name.rsplit(".", 1)[-1]
        if name.endswith(WN1):
            v = rng.standard_normal(shape) * 0.3
        elif name.endswith(WN0):
            # the row norm of the folded weight = the gain of the conv for unit-variance, uncorrelated inputs (silu halves the std)
            if ".ups." in name:
                u = h["upsample_rates"][int(name.split(".")[2])]
                gain = 2.3 * np.sqrt(u / 2.0) * np.sqrt(0.5)      # a row is one INPUT channel; 2 taps x cin rows reach an output sample
            elif "conv_pre" in name:
                gain = 1.0
            elif "conv_post" in name:
                gain = 0.7
            elif ".convs1." in name:
                gain = 1.2
            else:
                gain = 0.25
            v = gain * rng.uniform(0.75, 1.25, shape)
        elif leaf == "gamma":
            v = 0.5 * rng.uniform(0.5, 1.5, shape)
        elif leaf == "bias":
            v = 0.05 * rng.standard_normal(shape)
        elif ".norm." in name or name.startswith("backbone.norm") or (name.startswith("backbone.downsample_layers") and len(shape) == 1):
            v = 1.0 + 0.1 * rng.standard_normal(shape)            # LayerNorm weights
        elif "dwconv" in name:
            v = 0.4 * rng.standard_normal(shape)
        else:                                                      # stem, downsample and pointwise weights: fan-in scaled
            v = (0.5 if "pwconv" in name else 1.0) * rng.standard_normal(shape) / np.sqrt(np.prod(shape[1:]))
        sd[name] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return sd


def make_mel(B, T, M, seed):
    """A log-mel-like input: smooth along time and frequency plus noise, values around [-8, 2]."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[None, None, :]
    m = np.arange(M)[None, :, None]
    ph = rng.uniform(0, 2 * np.pi, (B, 1, 1))
    x = -3.0 + 2.5 * np.sin(0.37 * t + 0.11 * m + ph) * np.cos(0.05 * m + ph) + 1.0 * rng.standard_normal((B, M, T))
    return torch.from_numpy(x.astype(np.float32))


def rounder(dtype):
    """None -> identity; "f16" / "bf16" -> round to that format and back to float64."""
    if dtype is None:
        return lambda t: t
    td = {"f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    return lambda t: t.to(torch.float32).to(td).to(t.dtype)      # fp32 first, as on the device (fp32 values are what gets rounded)


def layer_norm(x, w, b):
    """Per frame over the channels of (B, C, T), eps 1e-6, biased variance (backbone.py:64-74)."""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    return w[None, :, None] * ((x - u) / torch.sqrt(s + 1e-6)) + b[None, :, None]


def fold(sd, p):
    """w = g v / ||v||, the norm over all dims but 0 (torch.nn.utils.parametrizations.weight_norm, dim=0)."""
    g, v = sd[p + WN0].double(), sd[p + WN1].double()
    return g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)


def prepare(sd, round_w=None, dtype=torch.float64, device="cpu"):
    """The tensors ``forward`` reads, made once: every parameter as `dtype` on `device`, the weight-normed convs folded (in float64)
    under ``<prefix>weight``, and the MFMA weights rounded by ``round_w``."""
    rw = rounder(round_w)
    out = {}
    for name, t in sd.items():
        if name.endswith(WN0):
            p = name[:-len(WN0)]
            w = fold(sd, p)
            out[p + "weight"] = (w if p == "head.conv_post." else rw(w)).to(device=device, dtype=dtype)
        elif name.endswith(WN1):
            continue
        else:
            mfma = name.endswith(".weight") and t.dim() >= 2 and "dwconv" not in name
            out[name] = (rw(t.double()) if mfma else t.double()).to(device=device, dtype=dtype)
    return out


def polyphase_weight(wt, u):
    """A ConvTranspose1d weight (Cin, Cout, 2u) with stride u, padding u / 2 as the weight (u * Cout, Cin, 3) of a 3-tap convolution
    (padding 1) whose output rows r * Cout + co at frame q are the samples t = u q + r: tap dq + 1 of row (r, co) is
    wt[ci, co, r + u / 2 - u dq] where that index is in [0, 2u), else 0 (the native kernels' map, ffgan_launch.h)."""
    cin, cout, k = wt.shape
    assert k == 2 * u
    w = torch.zeros(u * cout, cin, 3, dtype=wt.dtype)
    for r in range(u):
        for dq in (-1, 0, 1):
            j = r + u // 2 - u * dq
            if 0 <= j < k:
                w[r * cout:(r + 1) * cout, :, dq + 1] = wt[:, :, j].t()
    return w


def conv_transpose_polyphase(x, wt, bias, u):
    """F.conv_transpose1d(x, wt, bias, stride=u, padding=u // 2) for k = 2u through the 3-tap map: (B, Cin, L) -> (B, Cout, L * u)."""
    B, _, L = x.shape
    cout = wt.shape[1]
    y = F.conv1d(x, polyphase_weight(wt, u), None, padding=1)            # (B, u * Cout, L)
    y = y.view(B, u, cout, L).permute(0, 2, 3, 1).reshape(B, cout, L * u)
    return y if bias is None else y + bias[None, :, None]


def forward(sd, cfg, mel, round_w=None, round_x=None, prepared=None):
    """-> dict(audio (B, T * hop), pre_tanh (B, T * hop), encoder (B, D, T), levels [(B, C_i, L_i)] after every ParralelBlock) in float64."""
    W = prepared if prepared is not None else prepare(sd, round_w)       # prepared: its dtype and device are the computation's (tools/ffgan_bench.py)
    rx = rounder(round_x) if prepared is None else (lambda t: t)
    b, h = cfg["backbone"], cfg["head"]
    P = lambda n: W[n]      # noqa: E731
    K = b["kernel_size"]
    x = mel.to(W["backbone.norm.weight"])
    for i, C in enumerate(b["dims"]):
        ds = f"backbone.downsample_layers.{i}."
        if i == 0:
            x = F.conv1d(rx(x), P(ds + "0.weight"), P(ds + "0.bias"), padding=K // 2)
            x = layer_norm(x, P(ds + "1.weight"), P(ds + "1.bias"))
        else:
            x = layer_norm(x, P(ds + "0.weight"), P(ds + "0.bias"))
            x = F.conv1d(rx(x), P(ds + "1.weight"), P(ds + "1.bias"))
        for j in range(b["depths"][i]):
            p = f"backbone.stages.{i}.{j}."
            y = F.conv1d(x, P(p + "dwconv.weight"), P(p + "dwconv.bias"), padding=K // 2, groups=C)
            y = layer_norm(y, P(p + "norm.weight"), P(p + "norm.bias")).permute(0, 2, 1)
            y = F.linear(rx(y), P(p + "pwconv1.weight"), P(p + "pwconv1.bias"))
            y = F.gelu(y)
            y = F.linear(rx(y), P(p + "pwconv2.weight"), P(p + "pwconv2.bias"))
            x = x + (P(p + "gamma") * y).permute(0, 2, 1)
    enc = layer_norm(x, P("backbone.norm.weight"), P("backbone.norm.bias"))

    kp = h["pre_conv_kernel_size"]
    x = F.conv1d(rx(enc), P("head.conv_pre.weight"), P("head.conv_pre.bias"), padding=kp // 2)
    levels = []
    for i, u in enumerate(h["upsample_rates"]):
        k = h["upsample_kernel_sizes"][i]
        x = F.conv_transpose1d(rx(F.silu(x)), P(f"head.ups.{i}.weight"), P(f"head.ups.{i}.bias"), stride=u, padding=(k - u) // 2)
        outs = []
        for bi, (rk, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            y = x
            for p, d in enumerate(dil):
                p1, p2 = f"head.resblocks.{i}.blocks.{bi}.convs1.{p}.", f"head.resblocks.{i}.blocks.{bi}.convs2.{p}."
                t = F.conv1d(rx(F.silu(y)), P(p1 + "weight"), P(p1 + "bias"), dilation=d, padding=(rk * d - d) // 2)
                t = F.conv1d(rx(F.silu(t)), P(p2 + "weight"), P(p2 + "bias"), padding=(rk - 1) // 2)
                y = t + y
            outs.append(y)
        x = torch.stack(outs, dim=0).mean(dim=0)
        levels.append(x)
    ko = h["post_conv_kernel_size"]
    pre = F.conv1d(F.silu(x), P("head.conv_post.weight"), P("head.conv_post.bias"), padding=ko // 2).squeeze(1)
    return {"audio": torch.tanh(pre), "pre_tanh": pre, "encoder": enc, "levels": levels}


def rel_max(a, ref):
    """max |a - ref| / max |ref|."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())
