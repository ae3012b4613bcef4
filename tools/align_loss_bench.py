"""Device time and peak memory of the step behind the alignment search in training -- from the search's output to
(dur_loss, prior_loss, mu_y_masked) and back to (grad_mu_x, grad_logw, grad_fake_content) -- at the shape of BASELINE config 5
(B=64, Ty ragged U{600..1000}, Tx ragged U{100..350}, 80 mel channels; tools/mas_latency.py's shape), native against the torch
glue it replaces (models/model.py:162-176 on the dense alignment), on the same GPU in one process (developer tool; the
reference is not needed).

    python tools/align_loss_bench.py [--rounds 40] [--inner 50] [--warmup 5] [--out FILE]

Both arms start from what alignment.monotonic_alignment returns (the native arm from its durations, the torch arm from its
dense alignment and durations) and receive the same stand-in for the decoder's gradient of mu_y_masked.  The arms alternate
round by round; a round times `inner` forward + backward pairs between two HIP events that end in a synchronise; the figures are
medians over the rounds, with the quartiles beside them.  Peak memory is torch.cuda.max_memory_allocated over one forward +
backward pair of each arm above what was allocated before it; the dense alignment itself is reported separately (the search
still writes it; the native arm does not read it).
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    from stabletts_amd.alignment import align_and_losses, dense_alignment
    assert torch.cuda.is_available(), "align_loss_bench needs a HIP device"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(args.seed)
    B, M = 64, 80
    t_y = torch.randint(600, 1001, (B,), generator=gen)
    t_x = torch.randint(100, 351, (B,), generator=gen)
    Ty, Tx = int(t_y.max()), int(t_x.max())
    # a valid alignment: every token at least one frame, the rest spread at random (a few long tokens among many short ones)
    dur = torch.zeros(B, Tx, dtype=torch.int32)
    for b in range(B):
        n, extra = int(t_x[b]), int(t_y[b] - t_x[b])
        w = torch.rand(n, generator=gen) ** 4
        dur[b, :n] = 1 + torch.bincount(torch.multinomial(w, extra, replacement=True, generator=gen), minlength=n).to(torch.int32)
    assert torch.equal(dur.sum(1), t_y.to(torch.int32))
    x_mask = (torch.arange(Tx)[None] < t_x[:, None]).float().unsqueeze(1).to(dev)
    y_mask = (torch.arange(Ty)[None] < t_y[:, None]).float().unsqueeze(1).to(dev)
    mu_x0 = (torch.randn(B, M, Tx, generator=gen).to(dev) * x_mask)
    y = torch.randn(B, M, Ty, generator=gen).to(dev) * y_mask
    logw0 = torch.randn(B, 1, Tx, generator=gen).to(dev) * x_mask
    fake0 = torch.randn(1, M, 1, generator=gen).to(dev)
    g_masked = torch.randn(B, M, Ty, generator=gen).to(dev)                 # stands in for the decoder's grad_mu
    cfg_mask = (torch.rand(B, 1, generator=gen) > 0.2).to(dev)              # models/model.py:138
    x_lengths = t_x.to(dev)
    dur = dur.to(dev)
    durations = dur.to(torch.float32).unsqueeze(1)                           # monotonic_alignment's "durations"
    one = torch.ones((), device=dev)
    with torch.no_grad():
        tok = align_and_losses(mu_x0, x_mask, logw0, x_lengths, y, y_mask, dur)["frame_token"]
        attn = dense_alignment(tok, Tx).transpose(1, 2).contiguous().unsqueeze(1)      # (B, 1, Ty, Tx), as the search writes it
    leaves = lambda: [t.clone().requires_grad_(True) for t in (mu_x0, logw0, fake0)]   # noqa: E731

    def native():
        mu_x, logw, fake = leaves()
        o = align_and_losses(mu_x, x_mask, logw, x_lengths, y, y_mask, dur, keep=cfg_mask, fake_content=fake)
        torch.autograd.backward([o["mu_y_masked"], o["prior_loss"], o["dur_loss"]], [g_masked, one, one])
        return o["dur_loss"].detach(), o["prior_loss"].detach(), mu_x.grad, logw.grad, fake.grad

    def glue():
        mu_x, logw, fake = leaves()
        logw_ = torch.log(1e-8 + durations) * x_mask                                                   # :162
        dur_loss = torch.sum((logw - logw_) ** 2) / torch.sum(x_lengths)                               # :163
        a = attn.squeeze(1).transpose(1, 2)                                                            # :166
        mu_y = torch.matmul(a.squeeze(1).transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)        # :167-168
        cm = cfg_mask.unsqueeze(-1)                                                                    # :171
        mu_y_masked = mu_y * cm + ~cm * fake.repeat(mu_y.size(0), 1, mu_y.size(-1))                    # :172
        prior_loss = torch.sum(0.5 * ((y - mu_y) ** 2 + math.log(2 * math.pi)) * y_mask)               # :175
        prior_loss = prior_loss / (torch.sum(y_mask) * M)                                              # :176
        torch.autograd.backward([mu_y_masked, prior_loss, dur_loss], [g_masked, one, one])
        return dur_loss.detach(), prior_loss.detach(), mu_x.grad, logw.grad, fake.grad

    arms = {"native": native, "torch_glue": glue}
    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    res = dict(B=B, M=M, Ty=Ty, Tx=Tx, rounds=args.rounds, inner=args.inner, device=torch.cuda.get_device_name(0),
               dense_alignment_mbytes=round(attn.numel() * 4 / 1e6, 1), longest_token=int(dur.max()))
    # same results first (sums in another order differ in the last bits)
    rn, rg = native(), glue()
    for name, a, b in zip(("dur_loss", "prior_loss", "grad_mu_x", "grad_logw", "grad_fake_content"), rn, rg):
        res["max_diff_rel_" + name] = float((a.double() - b.double()).abs().max() / b.double().abs().max())
    del rn, rg
    for name, fn in arms.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        res[name + "_peak_extra_mbytes"] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
        del out
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():                      # the arms alternate within every round
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / args.inner)
    for name, v in ms.items():
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        res[name + "_ms"] = round(float(med), 4)
        res[name + "_ms_quartiles"] = [round(float(q1), 4), round(float(q3), 4)]
    res["native_over_torch"] = round(res["native_ms"] / res["torch_glue_ms"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
