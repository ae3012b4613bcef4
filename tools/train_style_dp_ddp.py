"""DistributedDataParallel around the natively trained MelStyleEncoder and DurationPredictor (native_training; tests/
test_gpu_style_duration_training.py runs it with 2 gloo ranks on one GPU and as one process on the whole batch).  Eval mode
(dropout off: the masks depend on the batch layout), plain SGD (updates linear in the reduced gradients: AdamW would turn the
rounding noise of near-zero gradients into full-size steps of random sign); loss = (sum(c * W) + the DP's masked squared error against fixed
targets / Tx) / items, each rank on its half of the batch.  Rank 0 saves the per-step losses and the parameters.

    python -m torch.distributed.run --nproc-per-node 2 tools/train_style_dp_ddp.py --out ddp.pt --backend gloo
    python tools/train_style_dp_ddp.py --out one.pt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Pair(torch.nn.Module):
    def __init__(self):
        super().__init__()
        import synth_weights as sw
        from stabletts_amd.duration_predictor_train import DurationPredictor
        from stabletts_amd.reference_encoder_train import MelStyleEncoder
        self.style = MelStyleEncoder(sw.N_MELS, style_vector_dim=sw.GIN, style_kernel_size=5, dropout=0.25)
        self.style.load_state_dict(sw.style_encoder_state_dict())
        self.dp = DurationPredictor(sw.DP_HIDDEN, sw.DP_FILTER, sw.DP_KERNEL, 0.5, sw.GIN)
        self.dp.load_state_dict(sw.duration_predictor_state_dict())

    def forward(self, y, ym, x, xm, w, target, per):
        c = self.style(y, ym)
        logw = self.dp(x, xm, c)
        T = x.shape[2]
        return (c * w).sum() / per + (((logw - target) ** 2) * xm).sum() / (per * T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    import synth_weights as sw
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group(args.backend, rank=rank, world_size=world)
    net = Pair().to(dev).eval()
    model = torch.nn.parallel.DistributedDataParallel(net, device_ids=[dev.index]) if world > 1 else net
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    B, T, Tx = 4, 80, 40
    y, ym = sw.style_inputs(B, T, [80, 61, 70, 33], 61)
    x, xm, _ = sw.dp_inputs(B, Tx, [40, 31, 22, 40], 62)
    rng = np.random.Generator(np.random.PCG64(63))
    w = rng.standard_normal((B, sw.GIN)).astype(np.float32)
    target = (1.5 + 0.3 * rng.standard_normal((B, 1, Tx))).astype(np.float32)
    per = B // world
    sl = slice(rank * per, (rank + 1) * per)
    batch = [torch.from_numpy(a[sl]).to(dev) for a in (y, ym, x, xm, w, target)]
    losses = []
    for _ in range(args.steps):
        opt.zero_grad()
        loss = model(*batch, per)      # DDP averages the ranks' gradients: each normalises by its own share
        loss.backward()
        opt.step()
        lv = loss.detach().clone()
        if world > 1:
            dist.all_reduce(lv)
            lv /= world
        losses.append(float(lv))
    if rank == 0:
        params = {k: v.detach().cpu() for k, v in net.named_parameters()}
        torch.save(dict(world=world, losses=losses, params=params), args.out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
