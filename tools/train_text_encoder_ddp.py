#!/usr/bin/env python
"""DDP training of the native text encoder AND the native CFM decoder in one model, in miniature (train.py:49-51,78-81 around
models/model.py:143-177): text encoder -> monotonic alignment search -> mu_y -> prior loss + the decoder's compute_loss, wrapped
in DistributedDataParallel, AdamW steps.  Two training engines share each rank's device and stream.

  python tools/train_text_encoder_ddp.py --out one.pt                                          (one process, whole batch)
  BENCH_SHARE_GPU=1 python -m torch.distributed.run --nproc-per-node 2 ... --out two.pt --backend gloo   (ranks share the GPU)

Every item has the same text length and the same total duration, so every rank's losses have the same normalisers: the mean
of the rank losses is the whole-batch loss and DDP's averaged gradient the whole-batch gradient.  Eval mode (dropout off), so
that the runs are comparable step by step.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_batch(B, Tx, seed):
    """tokens, lengths, c, y (B, 128, Ty) and y_mask: y follows the oracle encoder's mu_x expanded by fixed durations (1..3
    frames per token, the same pattern for every item) plus 0.3 noise -- a clear alignment for the search."""
    import oracle
    from oracle.make_golden_text_encoder import text_inputs
    tok, c, lens = text_inputs(B, Tx, [Tx] * B, seed)
    dur = np.array([1 + (i * 7 + 3) % 3 for i in range(Tx)])
    with torch.no_grad():
        _, mu_x, _ = oracle.text_encoder_forward(oracle.make_text_encoder_state_dict(2468), tok, c, lens)
    idx = torch.from_numpy(np.repeat(np.arange(Tx), dur))
    g = torch.Generator().manual_seed(seed)
    y = mu_x[:, :, idx] + 0.3 * torch.randn(B, 128, len(idx), generator=g)
    return tok, lens, c, y, torch.ones(B, 1, len(idx))


def chain_loss(x_mask, mu_x, y, y_mask, c, dec, t_rand, z):
    """models/model.py:148-177 from mu_x on (duration loss left out: the reference's DurationPredictor detaches x)."""
    from stabletts_amd.alignment import monotonic_alignment
    attn = monotonic_alignment(mu_x.detach(), x_mask, y, y_mask)["attn"]                 # (B, 1, Ty, Tx), no gradient
    mu_y = torch.matmul(attn.squeeze(1), mu_x.transpose(1, 2)).transpose(1, 2)
    diff_loss, _ = dec.compute_loss(y, y_mask, mu_y, c, t_rand=t_rand, z=z)
    prior = torch.sum(0.5 * ((y - mu_y) ** 2 + math.log(2 * math.pi)) * y_mask) / (torch.sum(y_mask) * y.shape[1])
    return diff_loss + prior, attn


class Chain(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        import oracle
        from stabletts_amd.flow_matching import CFMDecoder
        from stabletts_amd.text_encoder import TextEncoder
        self.enc = TextEncoder(401, 128, 256, 1024, 4, 3, 3, 0.1, 256, operand_dtype=dtype)
        self.enc.load_state_dict(oracle.make_text_encoder_state_dict(2468))
        self.dec = CFMDecoder(128, 128, 256, 128, 1024, 4, 6, 3, 0.1, 256, operand_dtype=dtype)
        self.dec.estimator.load_state_dict(oracle.make_state_dict(1234))

    def forward(self, tok, lens, c, y, y_mask, t_rand, z):
        _, mu_x, x_mask = self.enc(tok, c, lens)
        return chain_loss(x_mask, mu_x, y, y_mask, c, self.dec, t_rand, z)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--backend", default="nccl")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--items", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--dtype", default="f16")
    args = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local % ndev if os.environ.get("BENCH_SHARE_GPU") == "1" else local)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    net = Chain(args.dtype).to(dev).eval()
    model = torch.nn.parallel.DistributedDataParallel(net, device_ids=[dev.index]) if world > 1 else net
    opt = torch.optim.AdamW(net.parameters(), lr=2e-4)
    B = args.items
    tok, lens, c, y, y_mask = make_batch(B, args.tokens, 91)
    gen = torch.Generator().manual_seed(5)
    per = B // world
    sl = slice(rank * per, (rank + 1) * per)
    losses = []
    for step in range(args.steps):
        t_rand = torch.rand(B, 1, 1, generator=gen); z = torch.randn(*y.shape, generator=gen)
        opt.zero_grad()
        loss = model(*(v[sl].to(dev) for v in (tok, lens, c, y, y_mask, t_rand, z)))
        loss.backward()
        opt.step()
        lv = loss.detach().clone()
        if world > 1:
            dist.all_reduce(lv); lv /= world
        losses.append(float(lv))
    if rank == 0:
        keep = ["enc.emb.weight", "enc.encoder.0.attn.conv_v.weight", "enc.encoder.2.mlp.conv_2.weight", "enc.encoder.1.adaLN_modulation.2.weight",
                "enc.proj.weight", "dec.estimator.final_proj.weight", "dec.estimator.blocks.0.block.attn.conv_v.weight"]
        params = {k: v.detach().cpu() for k, v in net.named_parameters() if k in keep}
        torch.save(dict(world=world, losses=losses, params=params), args.out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
