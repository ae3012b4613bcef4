#!/usr/bin/env python
"""Throughput of the native Vocos vocoder (developer tool): mel (B, 128, T) -> audio, seconds of 44.1 kHz audio per
second and the per-class kernel times.  python tools/vocos_bench.py [B] [T] [dtype]
python tools/vocos_bench.py --ragged [dtype]: a bucket of 32 utterances of U{600..1000} frames (fixed seed) as the padded dense
call, the ragged call and a loop of 32 single-utterance calls, and the ragged call with every length equal to T beside the dense
call; writes profiles/vocos_ragged_bench.txt."""
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
argv = [a for a in sys.argv if a != "--ragged"]
B = int(argv[1]) if len(argv) > 1 and not ragged else 32
T = int(argv[2]) if len(argv) > 2 and not ragged else 1000
dt = (argv[1] if len(argv) > 1 else "f16") if ragged else (argv[3] if len(argv) > 3 else "f16")
c = vo.VocosConfig
m = Vocos(types.SimpleNamespace(input_channels=c.input_channels, dim=c.dim, intermediate_dim=c.intermediate_dim, num_layers=c.num_layers),
          types.SimpleNamespace(n_fft=c.n_fft, hop_length=c.hop_length), operand_dtype=dt)
m.load_state_dict({k: torch.from_numpy(v) for k, v in vo.make_vocos_state_dict(77).items()})
m = m.cuda()


def ragged_leg():
    """Medians over ROUNDS rounds; in a round every leg runs CALLS times between two synchronisations, the legs in turn, so
    that drift of the shared machine lands on all of them.  Host clock around work that ends in a device synchronise."""
    ROUNDS, CALLS, NB = 15, 5, 32
    lengths = np.random.default_rng(4).integers(600, 1001, NB).tolist()
    Tmax, rows = max(lengths), sum(lengths)
    mel = torch.from_numpy(vo.make_mel(NB, Tmax, 3)).cuda()
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
        {"workload": "vocos_bucket", "dtype": dt, "B": NB, "Tmax": Tmax, "packed_rows": rows, "padded_rows": NB * Tmax,
         "rows_ratio": round(rows / (NB * Tmax), 3), "rounds": ROUNDS, "calls_per_round": CALLS,
         "dense_padded_ms_median": round(med["dense_padded"], 3), "ragged_ms_median": round(med["ragged"], 3),
         "solo_loop_ms_median": round(med["solo_loop"], 3), "ragged_over_dense": round(med["ragged"] / med["dense_padded"], 3),
         "ragged_over_solo_loop": round(med["ragged"] / med["solo_loop"], 3)},
        {"workload": "vocos_equal_lengths", "dtype": dt, "B": NB, "T": Tmax, "rows": NB * Tmax,
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
    with open(out, "w") as f:
        f.write(head)
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if ragged:
    ragged_leg()
    sys.exit(0)
mel = torch.from_numpy(vo.make_mel(B, T, 3)).cuda()
for _ in range(3):
    m(mel)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(10):
    m(mel)
torch.cuda.synchronize(); ms = (time.perf_counter() - t0) / 10 * 1e3
eng = m.engine(); eng.profile_enable(True); m(mel); torch.cuda.synchronize()
pr = eng.profile_read(); eng.profile_enable(False)
flops = B * T * (2 * 896 * 512 + 8 * 4 * 512 * 1536 + 2 * 512 * 2050)
print(json.dumps({"B": B, "T": T, "dtype": dt, "ms": round(ms, 3), "frames_per_s": round(B * T / ms * 1e3),
                  "audio_s_per_s": round(B * T * 512 / 44100 / ms * 1e3, 1), "gemm_tflops": round(flops / ms / 1e9, 1),
                  "classes_ms": {k: round(v["total_ms"], 3) for k, v in pr.items() if v["launches"]}}))
