#!/usr/bin/env python
"""Workload for comparing the two families of row kernels at one width (developer tool), to be run under a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/vocos_row_kernels.py --dim 768

Runs, at 32 x 1000 frames dense and on tools/vocos_bench.py's ragged bucket (32 utterances of U{600..1000} frames), 5 calls each of
  * the Vocos vocoder at --dim (64 mel channels, intermediate_dim 256, 2 blocks): voc_ln_kernel and voc_dwconv_ln_kernel /
    voc_dwconv_ln_ragged_kernel, templated on channels per lane, 4 frames per wave;
  * a FireflyGAN vocoder whose ConvNeXt encoder is one stage of 2 blocks at the same width (hop 8 head): ffg_ln_kernel and
    ffg_dwconv_ln_kernel, run-time width, one frame per group.
Both depthwise kernels read the same fp32 rows [32000 or the bucket's][dim] and write the same 16-bit rows, so their average
durations in the trace's kernel statistics compare the kernels alone.  profiles/vocos_dims_bench.txt records the figures."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vocos_oracle as vo                                      # noqa: E402
from stabletts_amd.ffgan import FireflyGANBase                             # noqa: E402
from stabletts_amd.vocos import Vocos                                      # noqa: E402
from tests import ffgan_restatement as fr                                  # noqa: E402

dim = int(sys.argv[sys.argv.index("--dim") + 1])
CALLS, NB, M = 5, 32, 64
lengths = np.random.default_rng(4).integers(600, 1001, NB).tolist()

cfg = vo.vocos_config(input_channels=M, dim=dim, intermediate_dim=256, num_layers=2)
voc = Vocos(types.SimpleNamespace(input_channels=M, dim=dim, intermediate_dim=256, num_layers=2),
            types.SimpleNamespace(n_fft=cfg.n_fft, hop_length=cfg.hop_length))
voc.load_state_dict({k: torch.from_numpy(v) for k, v in vo.make_vocos_state_dict(77, cfg).items()})
voc = voc.cuda()
fcfg = fr.small_config(dims=(dim,), depths=(2,), mels=M)
ff = FireflyGANBase(config=fcfg)
ff.load_state_dict(fr.make_state_dict(fcfg, fr.SEED), strict=True)
ff = ff.cuda().eval()

mel = torch.from_numpy(vo.make_mel(NB, 1000, 3, M)).cuda()
with torch.inference_mode():
    for m in (voc, ff):
        for _ in range(CALLS):
            m(mel)
        for _ in range(CALLS):
            m.forward_ragged(mel, lengths)
torch.cuda.synchronize()
print(f"dim {dim}: {CALLS} dense calls at {NB} x 1000 frames and {CALLS} ragged calls at {sum(lengths)} packed rows, each vocoder")
