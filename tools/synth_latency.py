"""Per-stage device time of the native text -> mel chain of StableTTS.synthesise (models/model.py:79-108), and stages 1
and 3 (MelStyleEncoder, DurationPredictor) as stock torch.nn layers holding the same seeded weights on the same GPU
(developer tool; the reference tree is not needed: the torch restatement below is eval-mode reference_encoder.py:74-93 and
duration_predictor.py:24-37).  Times are medians of HIP events over --iters runs after --warmup.

    python tools/synth_latency.py [--iters 20] [--warmup 5]        -> one JSON line per shape (B=1 Tx=120, B=32 Tx=200; T_ref 600)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class TorchStyleEncoder(nn.Module):
    def __init__(self, sd):
        super().__init__()
        self.l0, self.l3 = nn.Linear(128, 128), nn.Linear(128, 128)
        self.c0, self.c1 = nn.Conv1d(128, 256, 5, padding=2), nn.Conv1d(128, 256, 5, padding=2)
        self.attn = nn.MultiheadAttention(128, 2, batch_first=True)
        self.fc = nn.Linear(128, 256)
        self.mish = nn.Mish()
        names = {"l0": "spectral.0", "l3": "spectral.3", "c0": "temporal.0.conv1", "c1": "temporal.1.conv1", "fc": "fc"}
        own = {f"{k}.{w}": sd[f"{v}.{w}"] for k, v in names.items() for w in ("weight", "bias")}
        own.update({"attn." + k[len("slf_attn."):]: v for k, v in sd.items() if k.startswith("slf_attn.")})
        self.load_state_dict(own, strict=True)

    def forward(self, y):
        x = self.mish(self.l3(self.mish(self.l0(y.transpose(1, 2))))).transpose(1, 2)
        for conv in (self.c0, self.c1):
            a, g = conv(x).chunk(2, dim=1)
            x = x + a * torch.sigmoid(g)
        x = x.transpose(1, 2)
        x, _ = self.attn(x, x, x, need_weights=False)
        return self.fc(x).mean(dim=1)


class TorchDurationPredictor(nn.Module):
    def __init__(self, sd):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv1d(256, 1024, 3, padding=1), nn.Conv1d(1024, 1024, 3, padding=1)
        self.norm1, self.norm2 = nn.LayerNorm(1024), nn.LayerNorm(1024)
        self.proj, self.cond = nn.Conv1d(1024, 1, 1), nn.Conv1d(256, 256, 1)
        self.load_state_dict(sd, strict=True)

    def forward(self, x, m, g):
        x = x + self.cond(g.unsqueeze(2))
        x = self.norm1(torch.relu(self.conv1(x * m)).transpose(1, 2)).transpose(1, 2)
        x = self.norm2(torch.relu(self.conv2(x * m)).transpose(1, 2)).transpose(1, 2)
        return self.proj(x * m) * m


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import oracle
    from tests import synth_weights as sw
    from stabletts_amd.alignment import length_regulate
    from stabletts_amd.duration_predictor import DurationPredictor
    from stabletts_amd.flow_matching import CFMDecoder
    from stabletts_amd.reference_encoder import MelStyleEncoder
    from stabletts_amd.text_encoder import TextEncoder
    torch.set_grad_enabled(False)
    se_sd, dp_sd = sw.style_encoder_state_dict(), sw.duration_predictor_state_dict()
    se = MelStyleEncoder(128, style_vector_dim=256, style_kernel_size=5, dropout=0.25)
    se.load_state_dict(se_sd)
    enc = TextEncoder(401, 128, 256, 1024, 4, 3, 3, 0.1, 256)
    enc.load_state_dict(oracle.make_text_encoder_state_dict(2468))
    dp = DurationPredictor(256, 1024, 3, 0.5, 256)
    dp.load_state_dict(dp_sd)
    dec = CFMDecoder(128, 128, 256, 128, 1024, 4, 6, 3, 0.1, 256)
    dec.estimator.load_state_dict(oracle.make_state_dict(1234))
    se, enc, dp, dec = se.cuda(), enc.cuda(), dp.cuda(), dec.cuda()
    tse, tdp = TorchStyleEncoder(se_sd).cuda().eval(), TorchDurationPredictor(dp_sd).cuda().eval()
    fs, fc = (t.cuda() for t in oracle.make_cfg_params(4321))
    kw = dict(fake_speaker=fs, fake_content=fc, cfg_strength=3.0)
    for B, Tx, Tref in ((1, 120, 600), (32, 200, 600)):
        rng = np.random.Generator(np.random.PCG64(B))
        tok = torch.from_numpy(rng.integers(1, 401, size=(B, Tx))).cuda()
        lens = torch.full((B,), Tx, dtype=torch.long, device="cuda")
        y = torch.from_numpy((rng.standard_normal((B, 128, Tref)) * 2 - 5).astype(np.float32)).cuda()
        c = se(y)
        h, mu_x, xm = enc(tok, c, lens)
        logw = dp(h, xm, c)
        r = length_regulate(logw, xm, mu_x, 1.0, return_attn=False)
        res = {"B": B, "Tx": Tx, "T_ref": Tref, "Ty": int(r["y_lengths"].max())}
        res["native_ms"] = {
            "style_encoder": timed(lambda: se(y), args.iters, args.warmup),
            "text_encoder": timed(lambda: enc(tok, c, lens), args.iters, args.warmup),
            "duration_predictor": timed(lambda: dp(h, xm, c), args.iters, args.warmup),
            "length_regulate": timed(lambda: length_regulate(logw, xm, mu_x, 1.0, return_attn=False), args.iters, args.warmup),
            "decoder_euler10_cfg3": timed(lambda: dec(r["mu_y"], r["y_mask"], 10, 1.0, c, "euler", kw), max(3, args.iters // 4), 1),
        }
        res["torch_nn_ms"] = {"style_encoder": timed(lambda: tse(y), args.iters, args.warmup),
                              "duration_predictor": timed(lambda: tdp(h, xm, c), args.iters, args.warmup)}
        res["torch_vs_native_max_abs"] = {"c": float((tse(y) - c).abs().max()), "logw": float((tdp(h, xm, c) - logw).abs().max())}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
