#!/usr/bin/env python
"""Throughput of the native Vocos vocoder (developer tool): mel (B, 128, T) -> audio, seconds of 44.1 kHz audio per
second and the per-class kernel times.  python tools/vocos_bench.py [B] [T] [dtype]
python tools/vocos_bench.py --ragged [dtype]: a bucket of 32 utterances of U{600..1000} frames (fixed seed) as the padded dense
call, the ragged call and a loop of 32 single-utterance calls, and the ragged call with every length equal to T beside the dense
call; writes profiles/vocos_ragged_bench.txt (at the preset only).
--dim D --intermediate-dim F --num-layers L (any of them; default the inference preset 512 / 1536 / 8): another generator, e.g. the
Vocos trainer's own 768 / 2048 / 12 (vocoders/vocos/config.py:21-26).  --torch: beside the native call, the same forward written in
torch ops (tests/vocos_vjp_restatement.torch_vocos) on the same GPU in fp32 and under fp16 autocast, the three legs in turn.
--n-fft N --hop-length H --input-channels M: another ISTFT size and mel width (n_fft 256 / 512 / 1024 / 2048 with hop n_fft / 4, M a
multiple of 16 up to 192), e.g. a 22.05 kHz model's --n-fft 1024 --hop-length 256 --input-channels 80; for the dense and the
--ragged leg.  --sample-rate R (default 44100; 22050 is usual for n_fft 1024, 16000 for 512) only scales audio_s_per_s."""
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vocos_oracle as vo                 # noqa: E402  (seeded weights / inputs only)
from stabletts_amd.vocos import Vocos                 # noqa: E402

ragged = "--ragged" in sys.argv
with_torch = "--torch" in sys.argv
argv = [a for a in sys.argv if a not in ("--ragged", "--torch")]
over = {}
for flag, key in (("--dim", "dim"), ("--intermediate-dim", "intermediate_dim"), ("--num-layers", "num_layers"), ("--n-fft", "n_fft"),
                  ("--hop-length", "hop_length"), ("--input-channels", "input_channels"), ("--sample-rate", "sample_rate")):
    if flag in argv:
        i = argv.index(flag)
        over[key] = int(argv[i + 1])
        del argv[i:i + 2]
B = int(argv[1]) if len(argv) > 1 and not ragged else 32
T = int(argv[2]) if len(argv) > 2 and not ragged else 1000
dt = (argv[1] if len(argv) > 1 else "f16") if ragged else (argv[3] if len(argv) > 3 else "f16")
sample_rate = over.pop("sample_rate", 44100)
c = vo.vocos_config(**over)
sd = vo.make_vocos_state_dict(77, c)
m = Vocos(types.SimpleNamespace(input_channels=c.input_channels, dim=c.dim, intermediate_dim=c.intermediate_dim, num_layers=c.num_layers),
          types.SimpleNamespace(n_fft=c.n_fft, hop_length=c.hop_length), operand_dtype=dt)
m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
m = m.cuda()


def ragged_leg():
    """Medians over ROUNDS rounds; in a round every leg runs CALLS times between two synchronisations, the legs in turn, so
    that drift of the shared machine lands on all of them.  Host clock around work that ends in a device synchronise."""
    ROUNDS, CALLS, NB = 15, 5, 32
    lengths = np.random.default_rng(4).integers(600, 1001, NB).tolist()
    Tmax, rows = max(lengths), sum(lengths)
    mel = torch.from_numpy(vo.make_mel(NB, Tmax, 3, c.input_channels)).cuda()
    for b, n in enumerate(lengths):
        mel[b, :, n:] = 0.0
    solo = [mel[b:b + 1, :, :n].contiguous() for b, n in enumerate(lengths)]
    full = [Tmax] * NB
    legs = {"dense_padded": lambda: m(mel), "ragged": lambda: m.forward_ragged(mel, lengths),
            "solo_loop": lambda: [m(x) for x in solo],
            "dense_a": lambda: m(mel), "ragged_equal_lengths": lambda: m.forward_ragged(mel, full), "dense_b": lambda: m(mel)}
    for fn in legs.values():          # every shape of the timed window, twice
        fn(); fn()
    ms = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize(); ms[k].append((time.perf_counter() - t0) / CALLS * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = abs(med["dense_a"] - med["dense_b"]) / med["dense_a"]
    lines = [
        {"workload": "vocos_bucket", "dtype": dt, "n_fft": c.n_fft, "hop_length": c.hop_length, "input_channels": c.input_channels, "dim": c.dim, "intermediate_dim": c.intermediate_dim, "num_layers": c.num_layers, "B": NB, "Tmax": Tmax, "packed_rows": rows, "padded_rows": NB * Tmax,
         "rows_ratio": round(rows / (NB * Tmax), 3), "rounds": ROUNDS, "calls_per_round": CALLS,
         "dense_padded_ms_median": round(med["dense_padded"], 3), "ragged_ms_median": round(med["ragged"], 3),
         "solo_loop_ms_median": round(med["solo_loop"], 3), "ragged_over_dense": round(med["ragged"] / med["dense_padded"], 3),
         "ragged_over_solo_loop": round(med["ragged"] / med["solo_loop"], 3)},
        {"workload": "vocos_equal_lengths", "dtype": dt, "dim": c.dim, "B": NB, "T": Tmax, "rows": NB * Tmax,
         "dense_a_ms_median": round(med["dense_a"], 3), "dense_b_ms_median": round(med["dense_b"], 3),
         "ragged_equal_lengths_ms_median": round(med["ragged_equal_lengths"], 3),
         "dense_run_to_run": round(spread, 4), "ragged_over_dense_a": round(med["ragged_equal_lengths"] / med["dense_a"], 4)},
    ]
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vocos_ragged_bench.txt")
    head = ("# tools/vocos_bench.py --ragged on one MI355X: one bucket of 32 utterances of U{600..1000} frames (seed 4) through the native\n"
            "# vocoder as the padded dense call (Vocos.forward: wrong for every utterance shorter than the longest), the ragged call\n"
            "# (Vocos.forward_ragged) and a loop of 32 single-utterance dense calls; and the ragged call with every length equal to T beside two\n"
            "# runs of the dense call at the same rows (their difference is the run-to-run spread).  ms per call, host clock around\n"
            "# calls_per_round calls ending in a device synchronise, legs in turn within a round, median over the rounds.\n")
    for ln in lines:
        print(json.dumps(ln))
    if over:          # the file records the preset
        return
    with open(out, "w") as f:
        f.write(head)
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if ragged:
    ragged_leg()
    sys.exit(0)
mel = torch.from_numpy(vo.make_mel(B, T, 3, c.input_channels)).cuda()
for _ in range(3):
    m(mel)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(10):
    m(mel)
torch.cuda.synchronize(); ms = (time.perf_counter() - t0) / 10 * 1e3
eng = m.engine(); eng.profile_enable(True); m(mel); torch.cuda.synchronize()
pr = eng.profile_read(); eng.profile_enable(False)
flops = B * T * (2 * 7 * c.input_channels * c.dim + c.num_layers * 4 * c.dim * c.intermediate_dim + 2 * c.dim * (c.n_fft + 2))
extra = {}
if with_torch:      # the torch statement of the same forward on the same GPU, the legs in turn (medians of 7 rounds of 3 calls)
    from tests.vocos_vjp_restatement import torch_vocos
    tp = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}

    def t_fp32():
        with torch.no_grad():
            return torch_vocos(tp, mel, c.num_layers, c.n_fft, c.hop_length)

    def t_fp16():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return torch_vocos(tp, mel, c.num_layers, c.n_fft, c.hop_length)
    legs = {"native": lambda: m(mel), "torch_fp32": t_fp32, "torch_fp16_autocast": t_fp16}
    for fn in legs.values():
        fn(); fn()
    torch.cuda.synchronize()
    extra["torch_fp16_autocast_vs_torch_fp32_max_rel"] = float((t_fp16().float() - t_fp32()).abs().max() / t_fp32().abs().max())
    times = {k: [] for k in legs}
    for _ in range(7):
        for k, fn in legs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(3):
                fn()
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) / 3 * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    extra = {**extra, "legs_ms_median": {k: round(v, 3) for k, v in med.items()},
             "torch_fp32_over_native": round(med["torch_fp32"] / med["native"], 2),
             "torch_fp16_autocast_over_native": round(med["torch_fp16_autocast"] / med["native"], 2)}
print(json.dumps({"B": B, "T": T, "dtype": dt, "n_fft": c.n_fft, "hop_length": c.hop_length, "input_channels": c.input_channels, "dim": c.dim, "intermediate_dim": c.intermediate_dim, "num_layers": c.num_layers, "ms": round(ms, 3), **extra, "frames_per_s": round(B * T / ms * 1e3),
                  "audio_s_per_s": round(B * T * c.hop_length / sample_rate / ms * 1e3, 1), "gemm_tflops": round(flops / ms / 1e9, 1),
                  "classes_ms": {k: round(v["total_ms"], 3) for k, v in pr.items() if v["launches"]}}))
