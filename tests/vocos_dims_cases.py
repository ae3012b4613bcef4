"""Cases of tests/golden/vocos_dims.npz (tools/make_golden_vocos_dims.py): the Vocos generator at backbone widths 768 and 1024 and
at the configuration the reference's Vocos trainer builds (vocoders/vocos/config.py:21-26: 128 / 768 / 2048 / 12).  Test
infrastructure shared by the generator and by tests/test_vocos_dims_cpu.py, test_gpu_vocos_dims.py and
test_gpu_vocos_dims_training.py; the layout follows tests/vocos_vjp_restatement.py's frames fixture.
"""
import numpy as np

from tests import vocos_vjp_restatement as R

TRAINER = dict(input_channels=128, dim=768, intermediate_dim=2048, num_layers=12)      # vocoders/vocos/config.py:21-26

# name -> (config fields, B, T, weight seed, mel seed, loss)
CASES = {
    "d768": (dict(input_channels=64, dim=768, intermediate_dim=256, num_layers=2), 3, 7, 121, 122, "linear"),
    "d1024": (dict(input_channels=64, dim=1024, intermediate_dim=256, num_layers=2), 3, 7, 131, 132, "linear"),
    "trainer": (TRAINER, 1, 4, 141, 142, "linear"),
}
# elements kept of every parameter gradient (whole up to this many): 116 tensors at 12 layers, so the trainer's case keeps fewer
KEEP = {"d768": 256, "d1024": 256, "trainer": 128}


def stored_elements(case, name_index, g, seed):
    """What the fixture keeps of gradient ``g`` of ``case``: all of it up to KEEP[case] elements, else fixed sampled elements."""
    g = np.asarray(g).reshape(-1)
    k = KEEP[case]
    return g if g.size <= k else g[R.sample_index(g.size, seed + name_index, k)]
