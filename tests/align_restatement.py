"""Plain torch-CPU restatement of length regulation (the reference's models/model.py:17-27 and :83-95): duration -> path -> mu_y,
in the same fp32 arithmetic, so that tests can check widths the committed fixture (tests/golden/align_outputs.npz) does not hold.
tests/test_align_sweep_cpu.py pins it bit for bit to every case of that fixture.

    path = generate_path(duration, mask)                 # duration (B, Tx), mask (B, Tx, Ty) -> (B, Tx, Ty) of mask.dtype
    out = length_regulate(logw, x_mask, mu_x, scale)     # logw, x_mask (B, 1, Tx), mu_x (B, M, Tx) -> dict, see below

Not a test module."""
import torch


def generate_path(duration, mask):
    """Token i owns the frames j with cum[i - 1] <= j < cum[i], cum the running fp32 sum of the durations; times the mask."""
    Ty = mask.shape[2]
    cum = torch.cumsum(duration.to(torch.float32), 1)                        # sequential on the CPU, like the kernels' own sum
    frames = torch.arange(Ty, dtype=torch.float32)
    below = (frames[None, None, :] < cum[:, :, None]).to(mask.dtype)         # frame j lies before the end of token i
    before = torch.cat([torch.zeros_like(below[:, :1]), below[:, :-1]], 1)   # ... and before the end of token i - 1
    return (below - before) * mask


def length_regulate(logw, x_mask, mu_x, length_scale=1.0):
    """-> dict(w_ceil (B, 1, Tx), y_lengths (B,) long, y_mask (B, 1, Ty), attn (B, Tx, Ty), mu_y (B, M, Ty)), Ty = max(y_lengths).
    mu_y is the gather that attn^T mu_x is: attn has at most one 1 per frame, and a product with 0 / 1 is exact."""
    w_ceil = torch.ceil(torch.exp(logw) * x_mask) * length_scale
    y_lengths = torch.clamp_min(w_ceil.sum((1, 2)), 1).long()
    Ty = int(y_lengths.max())
    y_mask = (torch.arange(Ty)[None, :] < y_lengths[:, None]).unsqueeze(1).to(x_mask.dtype)
    attn = generate_path(w_ceil[:, 0], x_mask[:, 0, :, None] * y_mask[:, 0, None, :])
    assert float(attn.sum(1).max()) <= 1 and float(attn.min()) >= 0
    token = attn.argmax(1)                                                   # (B, Ty)
    covered = attn.sum(1) > 0
    mu_y = torch.gather(mu_x, 2, token[:, None, :].expand(-1, mu_x.shape[1], -1)) * covered[:, None, :].to(mu_x.dtype)
    return dict(w_ceil=w_ceil, y_lengths=y_lengths, y_mask=y_mask, attn=attn, mu_y=mu_y)


def margin_from_integers(logw, x_mask):
    """The smallest relative distance of a float64 exp(logw) from an integer over the unmasked elements: while it is far above
    one fp32 ulp, ceil cannot depend on the last bit of anybody's expf."""
    w = torch.exp(logw.double())[x_mask != 0]
    return float(((w - torch.round(w)).abs() / w).min())
