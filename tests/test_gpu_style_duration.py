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


# ---- error behaviour of the C ABI across the six kinds of handle -----------------------------------------------------------
# (entry point, what it was called with) -> (code, st_last_error), recorded from the library as it was before the six kinds shared
# their handle plumbing; every build since must answer the same.  "another kind": a finalized handle of each of the five other
# kinds (one row where they all get the same answer, else a row per kind); "unfinalized": the entry point's own kind before
# st_finalize; "null": its own kind, finalized, first tensor null; "dropout": p_dropout = 1.5; "B = 0"; "stale": a backward with
# another forward's serial.
_ERROR_TABLE = {('st_estimator_forward', 'another kind'): (-3, 'this handle is not a CFM decoder (st_create)'),
 ('st_estimator_forward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading parameters'),
 ('st_estimator_forward', 'null'): (-1, 'null tensor pointer'),
 ('st_cfm_solve', 'another kind'): (-3, 'this handle is not a CFM decoder (st_create)'),
 ('st_cfm_solve', 'unfinalized'): (-3, 'st_finalize() has not been called after loading parameters'),
 ('st_cfm_solve', 'null'): (-1, 'null tensor pointer'),
 ('st_train_forward', 'another kind'): (-3, 'this handle is not a CFM decoder (st_create)'),
 ('st_train_forward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading parameters'),
 ('st_train_forward', 'null'): (-1, 'null tensor pointer'),
 ('st_train_forward', 'dropout'): (-1, 'p_dropout must be in [0, 1)'),
 ('st_text_encoder_forward', 'another kind'): (-3, 'this handle is not a text encoder (st_create_text_encoder)'),
 ('st_text_encoder_forward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading parameters'),
 ('st_text_encoder_forward', 'null'): (-1, 'null tensor pointer'),
 ('st_text_encoder_train_forward', 'another kind'): (-3, 'this handle is not a text encoder (st_create_text_encoder)'),
 ('st_text_encoder_train_forward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading parameters'),
 ('st_text_encoder_train_forward', 'null'): (-1, 'null tensor pointer'),
 ('st_text_encoder_train_forward', 'dropout'): (-1, 'p_dropout must be in [0, 1)'),
 ('st_vocos_forward', 'another kind'): (-3, 'this handle is not a vocoder (st_create_vocoder)'),
 ('st_vocos_forward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading parameters'),
 ('st_vocos_forward', 'null'): (-1, 'null tensor pointer'),
 ('st_vocos_forward', 'B = 0'): (-1, 'B and T must be >= 1'),
 ('st_style_encoder_forward', 'another kind'): (-3, 'this handle is not a style encoder (st_create_style_encoder)'),
 ('st_style_encoder_forward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading parameters'),
 ('st_style_encoder_forward', 'null'): (-1, 'null tensor pointer'),
 ('st_style_encoder_forward', 'B = 0'): (-1, 'B and T must be >= 1'),
 ('st_style_encoder_train_forward', 'another kind'): (-3, 'this handle is not a style encoder (st_create_style_encoder)'),
 ('st_style_encoder_train_forward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading parameters'),
 ('st_style_encoder_train_forward', 'null'): (-1, 'null tensor pointer'),
 ('st_style_encoder_train_forward', 'dropout'): (-1, 'p_dropout must be in [0, 1)'),
 ('st_style_encoder_train_backward', 'another kind'): (-3, 'this handle is not a style encoder (st_create_style_encoder)'),
 ('st_style_encoder_train_backward', 'unfinalized'): (-3, 'st_style_encoder_train_backward needs a preceding st_style_encoder_train_forward'),
 ('st_style_encoder_train_backward', 'null'): (-1, 'null tensor pointer'),
 ('st_style_encoder_train_backward', 'stale'): (-3, 'st_style_encoder_train_backward: the engine holds the activations of forward #1 (B=1, T=8), not of #2 (B=1, T=8)'),
 ('st_duration_predictor_forward', 'another kind'): (-3, 'this handle is not a duration predictor (st_create_duration_predictor)'),
 ('st_duration_predictor_forward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading parameters'),
 ('st_duration_predictor_forward', 'null'): (-1, 'null tensor pointer'),
 ('st_duration_predictor_forward', 'B = 0'): (-1, 'B and Tx must be >= 1'),
 ('st_duration_predictor_train_forward', 'another kind'): (-3, 'this handle is not a duration predictor (st_create_duration_predictor)'),
 ('st_duration_predictor_train_forward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading parameters'),
 ('st_duration_predictor_train_forward', 'null'): (-1, 'null tensor pointer'),
 ('st_duration_predictor_train_forward', 'dropout'): (-1, 'p_dropout must be in [0, 1)'),
 ('st_duration_predictor_train_backward', 'another kind'): (-3, 'this handle is not a duration predictor (st_create_duration_predictor)'),
 ('st_duration_predictor_train_backward', 'unfinalized'): (-3, 'st_duration_predictor_train_backward needs a preceding st_duration_predictor_train_forward'),
 ('st_duration_predictor_train_backward', 'null'): (-1, 'null tensor pointer'),
 ('st_duration_predictor_train_backward', 'stale'): (-3, 'st_duration_predictor_train_backward: the engine holds the activations of forward #1 (B=1, Tx=8), not of #2 (B=1, Tx=4)'),
 ('st_mel_forward', 'another kind'): (-3, 'this handle is not a mel extractor (st_create_mel_extractor)'),
 ('st_mel_forward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading the window / filter bank'),
 ('st_mel_forward', 'null'): (-1, 'null tensor pointer'),
 ('st_mel_backward', 'another kind'): (-3, 'this handle is not a mel extractor (st_create_mel_extractor)'),
 ('st_mel_backward', 'unfinalized'): (-3, 'st_finalize() has not been called after loading the window / filter bank'),
 ('st_mel_backward', 'null'): (-1, 'null tensor pointer'),
 ('st_train_backward', 'another kind'): (-3, 'st_train_backward needs a preceding st_train_forward (none held: never run, or invalidated by a parameter update)'),
 ('st_train_backward', 'unfinalized'): (-3, 'st_train_backward needs a preceding st_train_forward (none held: never run, or invalidated by a parameter update)'),
 ('st_train_backward', 'null'): (-3, 'st_train_backward needs a preceding st_train_forward (none held: never run, or invalidated by a parameter update)'),
 ('st_text_encoder_train_backward', 'another kind'): (-3,
                                                      'st_text_encoder_train_backward needs a preceding st_text_encoder_train_forward (none held: never run, or invalidated by a parameter '
                                                      'update)'),
 ('st_text_encoder_train_backward', 'unfinalized'): (-3,
                                                     'st_text_encoder_train_backward needs a preceding st_text_encoder_train_forward (none held: never run, or invalidated by a parameter '
                                                     'update)'),
 ('st_text_encoder_train_backward', 'null'): (-3,
                                              'st_text_encoder_train_backward needs a preceding st_text_encoder_train_forward (none held: never run, or invalidated by a parameter update)'),
 ('st_repack', 'decoder'): (0, ''),
 ('st_repack', 'text encoder'): (0, ''),
 ('st_repack', 'vocoder'): (-4, 'st_repack: vocoder handles re-pack through st_finalize'),
 ('st_repack', 'style encoder'): (-4, 'st_repack: style-encoder / duration-predictor handles read their parameters in place'),
 ('st_repack', 'duration predictor'): (-4, 'st_repack: style-encoder / duration-predictor handles read their parameters in place'),
 ('st_repack', 'mel extractor'): (-4, 'st_repack: mel-extractor handles re-read their filter bank through st_finalize'),
 ('st_train_serial', 'decoder'): (0, ''),
 ('st_train_serial', 'text encoder'): (0, ''),
 ('st_train_serial', 'vocoder'): (0, ''),
 ('st_train_serial', 'style encoder'): (1, ''),
 ('st_train_serial', 'duration predictor'): (1, ''),
 ('st_train_serial', 'mel extractor'): (0, ''),
 ('st_finalize', 'decoder, nothing loaded'): (-3, 'parameter not loaded: blocks.0.block.adaLN_modulation.2.bias'),
 ('st_finalize', 'text encoder, nothing loaded'): (-3, 'parameter not loaded: emb.weight'),
 ('st_finalize', 'vocoder, nothing loaded'): (-3, 'parameter not loaded: backbone.convnext.0.dwconv.bias'),
 ('st_finalize', 'style encoder, nothing loaded'): (-3, 'parameter not loaded: fc.bias'),
 ('st_finalize', 'duration predictor, nothing loaded'): (-3, 'parameter not loaded: cond.bias'),
 ('st_finalize', 'mel extractor, nothing loaded'): (-3, 'parameter not loaded: mel_scale.fb'),
 ('st_load_param', 'unknown name'): (-1, 'unexpected parameter name: conv9.weight'),
 ('st_load_param', 'shape'): (-1, 'shape mismatch for conv1.bias'),
 ('st_load_param', 'null'): (-1, 'null argument'),
 ('st_bind_param', 'unknown name'): (-1, 'unexpected parameter name: conv9.weight'),
 ('st_bind_param', 'shape'): (-1, 'shape mismatch for conv1.bias'),
 ('st_bind_param', 'null'): (-1, 'null argument')}


def _error_calls():
    """Builds one small handle of every kind twice (unfinalized / finalized with all-zero parameters) and returns
    {(entry, case): (code, message)} of bad calls.  No call gets as far as a launch except the two tiny training forwards
    whose activations the "stale" cases need."""
    import ctypes
    from stabletts_amd import _lib
    dit = (8, 256, 128, 4, 2, 3, 256)
    make = {
        "decoder": lambda: _lib.Engine(*dit),
        "text encoder": lambda: _lib.Engine(*dit, text_encoder_vocab=10),
        "vocoder": lambda: _lib.Engine(*dit, vocoder=dict(input_channels=64, dim=512, intermediate_dim=256, num_layers=1, n_fft=2048, hop_length=512)),
        "style encoder": lambda: _lib.Engine(*dit, style_encoder=dict(n_mel_channels=8, style_hidden=64, style_vector_dim=8, style_kernel_size=1, style_head=1)),
        "duration predictor": lambda: _lib.Engine(*dit, duration_predictor=dict(in_channels=8, filter_channels=128, kernel_size=1, gin_channels=8)),
        "mel extractor": lambda: _lib.Engine(*dit, mel=dict(n_fft=32, win_length=32, hop_length=8, pad=12, n_mels=4, center=0, pad_mode=0)),
    }
    raw = {k: f() for k, f in make.items()}
    fin = {k: f() for k, f in make.items()}
    for e in fin.values():
        e.load_state_dict({n: torch.zeros(s) for n, s in e.param_info()})
    lib = fin["decoder"].lib
    bufs = [torch.zeros(1 << 14, device="cuda") for _ in range(5)]
    p, q, r, s, t = (b.data_ptr() for b in bufs)
    # entry -> (own kind, call(handle, first tensor))
    entries = {
        "st_estimator_forward": ("decoder", lambda h, a: lib.st_estimator_forward(h, a, 1, q, r, s, t, p, 1, 8, None)),
        "st_cfm_solve": ("decoder", lambda h, a: lib.st_cfm_solve(h, a, q, r, s, 2, 0, 0, 0.0, None, None, t, 1, 8, None)),
        "st_train_forward": ("decoder", lambda h, a: lib.st_train_forward(h, a, q, r, s, t, p, 1, 8, 0.0, 0, None)),
        "st_text_encoder_forward": ("text encoder", lambda h, a: lib.st_text_encoder_forward(h, a, q, r, s, t, p, 1, 8, None)),
        "st_text_encoder_train_forward": ("text encoder", lambda h, a: lib.st_text_encoder_train_forward(h, a, q, r, s, t, p, 1, 8, 0.0, 0, None)),
        "st_vocos_forward": ("vocoder", lambda h, a: lib.st_vocos_forward(h, a, q, 1, 8, None)),
        "st_style_encoder_forward": ("style encoder", lambda h, a: lib.st_style_encoder_forward(h, a, None, q, 1, 8, None)),
        "st_style_encoder_train_forward": ("style encoder", lambda h, a: lib.st_style_encoder_train_forward(h, a, None, q, 1, 8, 0.0, 0, None)),
        "st_style_encoder_train_backward": ("style encoder", lambda h, a: lib.st_style_encoder_train_backward(h, 7, 1, 8, a, q, None)),
        "st_duration_predictor_forward": ("duration predictor", lambda h, a: lib.st_duration_predictor_forward(h, a, q, r, s, 1, 8, None)),
        "st_duration_predictor_train_forward": ("duration predictor", lambda h, a: lib.st_duration_predictor_train_forward(h, a, q, r, s, 1, 8, 0.0, 0, None)),
        "st_duration_predictor_train_backward": ("duration predictor", lambda h, a: lib.st_duration_predictor_train_backward(h, 7, 1, 8, a, q, None)),
        "st_mel_forward": ("mel extractor", lambda h, a: lib.st_mel_forward(h, a, 1, 64, q, None)),
        "st_mel_backward": ("mel extractor", lambda h, a: lib.st_mel_backward(h, a, q, 1, 64, 0, r, s, None)),
        "st_train_backward": ("decoder", lambda h, a: lib.st_train_backward(h, 7, 1, 8, a, None, None, None, None)),
        "st_text_encoder_train_backward": ("text encoder", lambda h, a: lib.st_text_encoder_train_backward(h, 7, 1, 8, a, None, None, None, None)),
    }
    got = {}

    def rec(key, e, rc):
        got[key] = (int(rc), lib.st_last_error(e.handle).decode() if rc < 0 else "")

    for name, (own, call) in entries.items():
        for kind, e in fin.items():
            if kind != own:
                rec((name, kind), e, call(e.handle, p))
        rec((name, "unfinalized"), raw[own], call(raw[own].handle, p))
        rec((name, "null"), fin[own], call(fin[own].handle, None))
        assert call(None, p) == _lib.ST_ERR_INVALID, name
    for name in ("st_train_forward", "st_text_encoder_train_forward"):
        own = entries[name][0]
        rec((name, "dropout"), fin[own], getattr(lib, name)(fin[own].handle, p, q, r, s, t, p, 1, 8, 1.5, 0, None))
    e = fin["style encoder"]
    rec(("st_style_encoder_train_forward", "dropout"), e, lib.st_style_encoder_train_forward(e.handle, p, None, q, 1, 8, 1.5, 0, None))
    rec(("st_style_encoder_forward", "B = 0"), e, lib.st_style_encoder_forward(e.handle, p, None, q, 0, 8, None))
    assert lib.st_style_encoder_train_forward(e.handle, p, None, q, 1, 8, 0.0, 0, None) == 0
    rec(("st_style_encoder_train_backward", "stale"), e, lib.st_style_encoder_train_backward(e.handle, 2, 1, 8, p, q, None))
    e = fin["duration predictor"]
    rec(("st_duration_predictor_train_forward", "dropout"), e, lib.st_duration_predictor_train_forward(e.handle, p, q, r, s, 1, 8, 1.5, 0, None))
    rec(("st_duration_predictor_forward", "B = 0"), e, lib.st_duration_predictor_forward(e.handle, p, q, r, s, 0, 8, None))
    assert lib.st_duration_predictor_train_forward(e.handle, p, q, r, s, 1, 8, 0.0, 0, None) == 0
    rec(("st_duration_predictor_train_backward", "stale"), e, lib.st_duration_predictor_train_backward(e.handle, 2, 1, 4, p, q, None))
    e = fin["vocoder"]
    rec(("st_vocos_forward", "B = 0"), e, lib.st_vocos_forward(e.handle, p, q, 0, 8, None))
    # st_repack says which kinds have something to re-pack; st_load_param / st_bind_param share their name and shape checks
    for kind, e in fin.items():
        rec(("st_repack", kind), e, lib.st_repack(e.handle, None))
        rec(("st_train_serial", kind), e, lib.st_train_serial(e.handle))
    for kind, e in raw.items():
        rec(("st_finalize", kind + ", nothing loaded"), e, lib.st_finalize(e.handle))
    e = raw["duration predictor"]
    for fn in ("st_load_param", "st_bind_param"):
        f = getattr(lib, fn)
        rec((fn, "unknown name"), e, f(e.handle, b"conv9.weight", p, (ctypes.c_int64 * 1)(128), 1))
        rec((fn, "shape"), e, f(e.handle, b"conv1.bias", p, (ctypes.c_int64 * 1)(127), 1))
        rec((fn, "null"), e, f(e.handle, b"conv1.bias", None, (ctypes.c_int64 * 1)(128), 1))
    torch.cuda.synchronize()
    for e in list(raw.values()) + list(fin.values()):
        e.close()
    return got


def test_bad_calls_answer_as_before_across_the_six_kinds():
    got = _error_calls()
    want = lambda k: _ERROR_TABLE[k] if k in _ERROR_TABLE else _ERROR_TABLE[(k[0], "another kind")]      # noqa: E731
    wrong = {k: (v, want(k)) for k, v in got.items() if v != want(k)}
    assert not wrong, wrong
    assert {k if k in _ERROR_TABLE else (k[0], "another kind") for k in got} == set(_ERROR_TABLE)      # every row was exercised
