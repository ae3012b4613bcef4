"""Native MelStyleEncoder and DurationPredictor (fp32 kernels) against the REAL reference modules, on a real MI355X:
tests/golden/synthesise_outputs.npz (tools/make_golden_synthesise.py) with the seeded weights of tests/synth_weights.py.
Gates: c max abs error / max|c| <= 1e-5 (measured <= 1.1e-6); logw max abs error <= 1e-4 on valid tokens and exactly 0 on padded ones;
w_ceil and y_lengths of length_regulate identical to the reference's.  Run with ``-m gpu``."""
import os

import numpy as np
import pytest
import torch

from tests import synth_weights as sw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "synthesise_outputs.npz")))


@pytest.fixture(scope="module")
def style():
    from stabletts_amd.reference_encoder import MelStyleEncoder
    m = MelStyleEncoder(sw.N_MELS, style_vector_dim=sw.GIN, style_kernel_size=5, dropout=0.25)
    m.load_state_dict(sw.style_encoder_state_dict(), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def dp():
    from stabletts_amd.duration_predictor import DurationPredictor
    m = DurationPredictor(sw.DP_HIDDEN, sw.DP_FILTER, sw.DP_KERNEL, 0.5, sw.GIN)
    m.load_state_dict(sw.duration_predictor_state_dict(), strict=True)
    return m.cuda()


@pytest.mark.parametrize("case", list(sw.STYLE_CASES))
def test_style_encoder_matches_reference(style, gold, case):
    B, T, lengths, seed = sw.STYLE_CASES[case]
    y, m = sw.style_inputs(B, T, lengths, seed)
    c = style(torch.from_numpy(y).cuda(), torch.from_numpy(m).cuda() if m is not None else None).cpu().numpy()
    ref = gold[case + "_c"]
    err = float(np.abs(c - ref).max() / np.abs(ref).max())
    print(f"{case}: c max abs err / max|c| = {err:.2e}")
    assert c.shape == ref.shape and err <= 1e-5          # measured <= 1.1e-6 (gate of the issue: 1e-3)


def test_style_encoder_all_masked_item_is_nan_like_the_reference(style):
    y, _ = sw.style_inputs(2, 9, None, 5)
    m = sw.mask_of(2, 9, [9, 0])
    c = style(torch.from_numpy(y).cuda(), torch.from_numpy(m).cuda()).cpu()
    assert torch.isfinite(c[0]).all() and torch.isnan(c[1]).all()


@pytest.mark.parametrize("case", list(sw.DP_CASES))
def test_duration_predictor_matches_reference(dp, gold, case):
    from stabletts_amd.alignment import length_regulate
    B, T, lengths, seed = sw.DP_CASES[case]
    x, m, g = (torch.from_numpy(a).cuda() for a in sw.dp_inputs(B, T, lengths, seed))
    logw = dp(x, m, g)
    lw, ref, mm = logw.cpu().numpy(), gold[case + "_logw"], m.cpu().numpy()
    err = float(np.abs(lw - ref)[mm > 0].max())
    print(f"{case}: logw max abs err on valid tokens = {err:.2e}")
    assert lw.shape == ref.shape and err <= 1e-4
    assert np.all(lw[mm == 0] == 0.0)
    r = length_regulate(logw, m, torch.zeros(B, 1, T, device="cuda"), 1.0, return_attn=False)
    assert np.array_equal(r["w_ceil"].cpu().numpy(), gold[case + "_w_ceil"])
    assert np.array_equal(r["y_lengths"].cpu().numpy(), gold[case + "_y_lengths"])


def test_grad_enabled_and_cpu_calls_raise(style, dp):
    y = torch.zeros(1, sw.N_MELS, 8, device="cuda")
    x, m, g = torch.zeros(1, sw.DP_HIDDEN, 8, device="cuda"), torch.ones(1, 1, 8, device="cuda"), torch.zeros(1, sw.GIN, device="cuda")
    with torch.enable_grad():
        with pytest.raises(NotImplementedError):
            style(y)
        with pytest.raises(NotImplementedError):
            dp(x, m, g)
    with pytest.raises(ValueError):
        style(y.cpu())
    with pytest.raises(ValueError):
        dp(x.cpu(), m.cpu(), g.cpu())
    from stabletts_amd.duration_predictor import DurationPredictor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DurationPredictor(sw.DP_HIDDEN, sw.DP_FILTER, 3, 0.5, sw.GIN)(x.cpu(), m.cpu(), g.cpu())


def test_unsupported_configs_fail_at_create():
    from stabletts_amd import _lib
    from stabletts_amd.duration_predictor import DurationPredictor
    from stabletts_amd.reference_encoder import MelStyleEncoder
    with pytest.raises(_lib.NativeError) as ei:
        DurationPredictor(256, 1000, 3, 0.5, 256).cuda().engine()
    assert ei.value.code == _lib.ST_ERR_UNSUPPORTED
    with pytest.raises(_lib.NativeError) as ei:
        MelStyleEncoder(128, style_head=4).cuda().engine()
    assert ei.value.code == _lib.ST_ERR_UNSUPPORTED


def test_entry_points_reject_other_kinds(style, dp):
    lib = style.engine().lib
    se, de = style.engine().handle, dp.engine().handle
    buf = torch.zeros(4096, device="cuda")
    p = buf.data_ptr()
    assert lib.st_style_encoder_forward(de, p, None, p, 1, 1, None) == _lib_state()
    assert lib.st_duration_predictor_forward(se, p, p, p, p, 1, 1, None) == _lib_state()
    assert lib.st_vocos_forward(se, p, p, 1, 1, None) == _lib_state()
    assert lib.st_text_encoder_forward(de, p, p, p, p, p, p, 1, 1, None) == _lib_state()
    assert lib.st_estimator_forward(se, p, 1, p, p, p, p, p, 1, 1, None) == _lib_state()
    assert lib.st_repack(de, None) == -4
    from stabletts_amd.vocos import Vocos
    import types
    voc = Vocos(types.SimpleNamespace(input_channels=128, dim=512, intermediate_dim=1536, num_layers=1),
                types.SimpleNamespace(n_fft=2048, hop_length=512)).cuda()
    assert lib.st_style_encoder_forward(voc.engine().handle, p, None, p, 1, 1, None) == _lib_state()
    assert lib.st_duration_predictor_forward(voc.engine().handle, p, p, p, p, 1, 1, None) == _lib_state()
    torch.cuda.synchronize()


def _lib_state():
    from stabletts_amd import _lib
    return _lib.ST_ERR_STATE
