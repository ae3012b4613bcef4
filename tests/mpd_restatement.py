"""Torch restatement of the multi-period discriminator and the three GAN losses of the Vocos training step (test
infrastructure, not part of the product): vocoders/vocos/models/discriminator.py:11-75 and loss.py:37-66, written as functions
of a dict of tensors so that they run in float64 on the CPU (the reference of the tests) and in fp32 on the GPU (the torch side
of the trajectory test and of tools/mpd_train_bench.py).  tests/test_mpd_cpu.py pins it to the float64 values and gradients of
the REAL module (tests/golden/mpd_grads.npz, tools/make_golden_mpd.py).

The forward is continuous but its gradient is not: the leaky ReLU picks a slope by sign and feature_loss takes |rl - gl|.  One
element that lands on the other side of zero in fp32 moves a gradient by 1e-4 .. 1e-2, far beyond rounding.  So every gradient
comparison is SIGN-CONSISTENT: ``forward`` writes the activation as pre * where(sign, 1, slope) and the L1 term as
((rl - gl) * sgn).mean(), with the signs either its own or supplied, and autograd yields the gradient of that branch pattern.
"""
import numpy as np
import torch
import torch.nn.functional as F

PERIODS = (2, 3, 5, 7, 11)
CHANNELS = (1, 32, 128, 512, 1024, 1024)       # before convs.i / after convs.(i - 1)
STRIDES = (3, 3, 3, 3, 1)
FULL_MAX = 512        # tensors up to this many elements are stored whole, larger ones as 512 sampled elements

# fixture cases (tools/make_golden_mpd.py)
LINEAR_CASES = {"linear_p3": (3, 2, 331, 101, 102), "linear_p11": (11, 2, 331, 111, 112)}      # period, B, T, weight seed, audio seed
TRAIN_STEP = dict(B=2, T=331, slope=0.1, seeds=(201, 202, 203, 204, 205, 206, 207, 208))         # first seed without a sign flip
# the second training-mode case of the GPU tests: the first seed of 301.. whose layer-0 pre-activations all stand more than
# 64 * 2^-24 * sum |terms| from zero in float64 (the test asserts it), so layer 0's signs are safe to share with the fp32 kernels
TRAIN_SMALL = dict(B=3, T=97, slope=0.1, seed=301)


def layer_names(i, prefix=""):
    """(g, v, bias) state-dict names of convs.i (i < 5) or conv_post (i = 5)."""
    base = prefix + (f"convs.{i}." if i < 5 else "conv_post.")
    return base + "parametrizations.weight.original0", base + "parametrizations.weight.original1", base + "bias"


def make_dp_state_dict(seed, prefix=""):
    """One DiscriminatorP: v ~ N(0, 1 / (Cin k)), g = ||v|| U(0.5, 1.5) (so g != ||v||: both weight-norm gradients are live),
    bias ~ U(-0.1, 0.1); float32, the reference's names and shapes."""
    rng = np.random.default_rng(seed)
    sd = {}
    for i in range(6):
        cin, cout, k = (CHANNELS[i], CHANNELS[i + 1], 5) if i < 5 else (CHANNELS[5], 1, 3)
        v = rng.standard_normal((cout, cin, k, 1)) / np.sqrt(cin * k)
        g = np.sqrt((v ** 2).sum(axis=(1, 2, 3), keepdims=True)) * rng.uniform(0.5, 1.5, (cout, 1, 1, 1))
        gn, vn, bn = layer_names(i, prefix)
        sd[bn] = rng.uniform(-0.1, 0.1, cout).astype(np.float32)
        sd[gn] = g.astype(np.float32)
        sd[vn] = v.astype(np.float32)
    return sd


def make_mpd_state_dict(seed, periods=PERIODS):
    sd = {}
    for k in range(len(periods)):
        sd.update(make_dp_state_dict(seed + 17 * k, f"discriminators.{k}."))
    return sd


def make_audio(B, T, seed):
    return (0.3 * np.random.default_rng(seed).standard_normal((B, 1, T))).astype(np.float32)


def loss_weights(shape, seed):
    """W of the linear loss sum(fmap * W)."""
    return np.random.default_rng(seed + 5000).standard_normal(shape).astype(np.float32)


def sample_index(numel, seed, k=512):
    rng = np.random.Generator(np.random.PCG64(seed + 9000))
    return np.unique(rng.integers(0, numel, size=min(k, numel)))


def stored_elements(index, g, seed):
    """What the fixture keeps of a tensor: all of it up to FULL_MAX elements, else the sampled elements."""
    g = np.asarray(g).reshape(-1)
    return g if g.size <= FULL_MAX else g[sample_index(g.size, seed + index)]


def rel_l2(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-300))


def to_torch(sd, dtype=torch.float64, device="cpu", requires_grad=False):
    return {k: torch.from_numpy(np.asarray(v)).to(device=device, dtype=dtype).requires_grad_(requires_grad) for k, v in sd.items()}


def weight_norm_w(v, g):
    """torch.nn.utils.parametrizations.weight_norm, dim 0: w = v g / ||v|| per output channel."""
    return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1))


def weight_norm_backward(dw, v, g):
    """The formula the native kernel implements: dg = <dw, v^>, dv = (g / ||v||) (dw - v^ dg), v^ = v / ||v||."""
    norm = v.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
    vhat = v / norm
    dg = (dw * vhat).flatten(1).sum(dim=1).view(-1, 1, 1, 1)
    return dg, (g / norm) * (dw - vhat * dg)


class Out:
    """fmaps: the five returned maps; signs: pre > 0 of layers 0..4 (own); margin0: min over layer 0 of |pre| / sum |terms|."""
    def __init__(self, fmaps, signs, margin0):
        self.fmaps, self.signs, self.margin0 = fmaps, signs, margin0


def forward(sd, x, period, slope, signs=None, prefix="", margin=True):
    """DiscriminatorP.forward on a dict of tensors.  x (B, 1, T).  signs: None (own) or five bool tensors (None entries: own).
    margin=False skips layer 0's margin (a second conv and a host read: the timed and the trajectory runs do without)."""
    b, c, t = x.shape
    if t % period != 0:
        n_pad = period - (t % period)
        x = F.pad(x, (0, n_pad), "reflect")
        t = t + n_pad
    x = x.view(b, c, t // period, period)
    fmaps, own, margin0 = [], [], None
    for i in range(5):
        gn, vn, bn = layer_names(i, prefix)
        w = weight_norm_w(sd[vn], sd[gn])
        pre = F.conv2d(x, w, sd[bn], stride=(STRIDES[i], 1), padding=(2, 0))
        if i == 0 and margin:
            with torch.no_grad():
                terms = F.conv2d(x.abs(), w.abs(), sd[bn].abs(), stride=(STRIDES[i], 1), padding=(2, 0))
                margin0 = float((pre.abs() / terms).min())
        own.append(pre.detach() > 0)
        sg = own[-1] if signs is None or signs[i] is None else signs[i]
        x = pre * torch.where(sg, torch.ones((), dtype=pre.dtype, device=pre.device), torch.full((), slope, dtype=pre.dtype, device=pre.device))
        if i > 0:
            fmaps.append(x)
    gn, vn, bn = layer_names(5, prefix)
    fmaps.append(F.conv2d(x, weight_norm_w(sd[vn], sd[gn]), sd[bn], stride=1, padding=(1, 0)))
    return Out(fmaps, own, margin0)


def linear_loss(fmaps, seed):
    """sum over the maps of sum(fmap * W): with slope 1 the whole network is linear, no branch exists."""
    return sum((f * torch.from_numpy(loss_weights(tuple(f.shape), seed + 31 * i)).to(device=f.device, dtype=f.dtype)).sum()
               for i, f in enumerate(fmaps))


def mpd_forward(sd, y, y_hat, slope, periods=PERIODS, signs=None, margin=True):
    """MultiPeriodDiscriminator.forward: per period the Out of cat([y, y_hat]) (its first half is the real signal's)."""
    x = torch.cat([y, y_hat], dim=0)
    return [forward(sd, x, p, slope, None if signs is None else signs[k], f"discriminators.{k}.", margin) for k, p in enumerate(periods)]


def gan_losses(outs, n, l1_signs=None):
    """discriminator_loss + feature_loss + generator_loss (loss.py:37-66) of mpd_forward's result, n = items of y.
    Returns (total, dict of the three, own L1 signs [period][map]: rl - gl > 0)."""
    disc = feat = gen = 0
    own = []
    for k, o in enumerate(outs):
        logits = torch.flatten(o.fmaps[-1], 1, -1)
        dr, dg = logits[:n], logits[n:]
        disc = disc + torch.mean((1 - dr) ** 2) + torch.mean(dg ** 2)
        gen = gen + torch.mean((1 - dg) ** 2)
        own.append([])
        for m, f in enumerate(o.fmaps):
            d = f[:n] - f[n:]
            own[-1].append(d.detach() > 0)
            sg = own[-1][-1] if l1_signs is None else l1_signs[k][m]
            sgn = torch.where(sg, torch.ones((), dtype=d.dtype, device=d.device), -torch.ones((), dtype=d.dtype, device=d.device))
            if l1_signs is None:
                sgn = torch.where(d.detach() == 0, torch.zeros((), dtype=d.dtype, device=d.device), sgn)     # torch.abs'(0) = 0
            feat = feat + torch.mean(d * sgn)
    feat = feat * 2
    return disc + feat + gen, dict(disc=disc, feat=feat, gen=gen), own
