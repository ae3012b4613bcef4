"""Device time of monotonic alignment search at the shape of BASELINE config 5 (B=64, Ty ragged U{600..1000}, Tx ragged
U{100..350}, D=80 mel channels), beside the host round trip the reference makes (developer tool; the reference is not
needed).  Times are medians of HIP events over --iters runs after --warmup.

    python tools/mas_latency.py [--iters 50] [--warmup 5]          -> one JSON line

  maximum_path_ms         the drop-in monotonic_align.maximum_path(neg_cent, mask): lengths from the mask, DP, backtrack, path
  mas_kernel_ms           st_maximum_path alone (lengths precomputed)
  neg_cent_ms             st_mas_neg_cent alone
  monotonic_alignment_ms  alignment.monotonic_alignment: neg_cent + lengths + DP + logw_
  ref_transfer_floor_ms   what the reference moves whatever its DP costs (monotonic_align/__init__.py:9-16): neg_cent.cpu(),
                          the mask sums to the host, and the int32 path back to the device as neg_cent.dtype.  The reference's
                          numba DP itself cannot run here (numba is not installed) and is not timed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    from stabletts_amd import alignment, monotonic_align
    assert torch.cuda.is_available(), "mas_latency needs a HIP device"
    gen = torch.Generator().manual_seed(args.seed)
    B, D = 64, 80
    t_y = torch.randint(600, 1001, (B,), generator=gen)
    t_x = torch.randint(100, 351, (B,), generator=gen)
    Ty, Tx = int(t_y.max()), int(t_x.max())
    dev = torch.device("cuda:0")
    x_mask = (torch.arange(Tx)[None] < t_x[:, None]).float().unsqueeze(1).to(dev)
    y_mask = (torch.arange(Ty)[None] < t_y[:, None]).float().unsqueeze(1).to(dev)
    mu_x = torch.randn(B, D, Tx, generator=gen).to(dev) * x_mask
    y = torch.randn(B, D, Ty, generator=gen).to(dev) * y_mask
    mask = (torch.unsqueeze(x_mask, 2) * torch.unsqueeze(y_mask, -1)).squeeze(1)       # models/model.py:157
    neg_cent = alignment.mas_neg_cent(mu_x, y)
    ty32, tx32 = t_y.to(dev, torch.int32), t_x.to(dev, torch.int32)

    def ref_transfer():
        host = neg_cent.data.cpu().numpy().astype(np.float32)
        path = np.zeros(host.shape, dtype=np.int32)
        mask.sum(1)[:, 0].data.cpu().numpy().astype(np.int32)
        mask.sum(2)[:, 0].data.cpu().numpy().astype(np.int32)
        return torch.from_numpy(path).to(device=dev, dtype=neg_cent.dtype)

    res = dict(B=B, Ty=Ty, Tx=Tx, D=D, cells_in_band=int(((t_y - t_x + 1) * t_x).sum()),
               neg_cent_mbytes=round(neg_cent.numel() * 4 / 1e6, 1),
               workspace_bytes=int(alignment._lib.load().st_maximum_path_workspace_bytes(B, Ty, Tx)))
    res["maximum_path_ms"] = timed(lambda: monotonic_align.maximum_path(neg_cent, mask), args.iters, args.warmup)
    res["mas_kernel_ms"] = timed(lambda: alignment.maximum_path(neg_cent, ty32, tx32), args.iters, args.warmup)
    res["neg_cent_ms"] = timed(lambda: alignment.mas_neg_cent(mu_x, y), args.iters, args.warmup)
    res["monotonic_alignment_ms"] = timed(lambda: alignment.monotonic_alignment(mu_x, x_mask, y, y_mask), args.iters, args.warmup)
    res["ref_transfer_floor_ms"] = timed(ref_transfer, max(5, args.iters // 5), 2)
    res["ref_dp"] = "not timed: numba is not installed"
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
