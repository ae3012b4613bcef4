"""Native Vocos generator training above 128 frames per batch (R = B * T > 128), on a real MI355X.

Every GEMM, LayerNorm and per-channel reduction of the training path runs over the flattened frames of the batch
(engine_vocos_train.cpp calls the fp32 tile kernels as B = 1, T = R).  tests/test_gpu_vocos_training.py stops at R = 122, where
the split-K weight gradient (fp32_tile.h: wgrad_split) still returns one plane, no lane of a per-channel reduction adds a second
frame and no grid-stride loop wraps; the reference trainer runs R = 32 x 40 = 1280.  The cases here are the smallest shapes that
reach those regions (CASES says which one each is for); each asserts on the host which paths it reaches before it compares.

Every case: weights make_vocos_state_dict(41), mel make_mel(seed 42), loss sum(audio * W) with W = loss_weights(seed 41); the
native audio, every parameter gradient (whole tensor) and d mel against the float64 restatement (tests/vocos_vjp_restatement.py,
computed once per shape), relative L2.  Bar: 4 x the largest fp32-torch-vs-float64 error the fixtures record for any parameter
gradient (vocos_grads.npz and vocos_grads_frames.npz), computed from the files.  Beside each native figure torch fp32's own error at the
same shape (torch_vocos under CPU autograd) is printed; it is no gate.  R1100 and preset_R260 also go against the REAL module's
float64 gradients (vocos_grads_frames.npz), per tensor 4 x that tensor's own fp32-torch error.  The head's clip at 100 IS
reached at R1100, R1600_M192 and R4100_F512; every case asserts that no log-magnitude lies within 1e-4 of ln 100.

NOT reached, and why:
  * col2im's grid-stride loop (M * R elements) wraps only from R = 10923 at M = 192: the head rows of such a batch alone are
    100 MB per buffer, too much for a test that has to stay within seconds.
  * the 32-plane cap of wgrad_split cannot be reached by this engine: its narrowest weight gradient (dim 512 x 64 n_mels x 7
    taps, or 512 x 256) has at least 32 tiles, so at most 8 planes are asked for.  The style / duration and period-discriminator
    tests reach the cap on the same kernel.
Run with ``-m gpu``.
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import vocos_oracle as vo
from tests import synth_weights as sw
from tests import vocos_vjp_restatement as R
from tests.test_gpu_vocos_training import SMALL, _linear_loss, _module, _rel_l2, _run

pytestmark = [pytest.mark.gpu, pytest.mark.grad]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WSEED, MSEED = 41, 42
WRAP = 8192 * 256           # elements above which a grid_1d(n, 8192) loop of 256 threads wraps

# id -> (config fields, B, T, {weight gradient: (planes, frames in the last plane)}, elementwise loops claimed to wrap)
CASES = {
    # first two-plane split; fs = 96: the last plane holds 33 frames, one full 32-frame chunk and a one-frame chunk
    "R129": (SMALL, 3, 43, {"head.out": (1, 129), "pwconv1": (2, 33), "pwconv2": (2, 33), "embed": (2, 33)}, {}),
    # lane 0 of every per-channel reduction adds a second frame; five 64-frame tiles, the last with one frame; three planes
    "R257_one_item": (SMALL, 1, 257, {"head.out": (1, 257), "pwconv1": (3, 65), "pwconv2": (3, 65), "embed": (3, 65)}, {}),
    # every conv tap but the centre masked at every frame, an item boundary at every frame, ISTFT with T = 1 per item
    "R257_items_of_one_frame": (SMALL, 257, 1, {"head.out": (1, 257), "pwconv1": (3, 65), "pwconv2": (3, 65), "embed": (3, 65)}, {}),
    # pwconv planes: 8 requested, 7 returned (fs = 160); items of 44 frames straddle tiles, chunks and plane boundaries
    "R1100": (SMALL, 25, 44, {"head.out": (1, 1100), "pwconv1": (7, 140), "pwconv2": (7, 140), "embed": (5, 204)}, {}),
    # the im2col loop wraps; embed: 2 planes over a 1344-wide N (21 column tiles)
    "R1600_M192": ({**SMALL, "input_channels": 192}, 2, 800,
                   {"head.out": (1, 1600), "pwconv1": (8, 32), "pwconv2": (8, 32), "embed": (2, 800)}, {"im2col (7 M R)": 7 * 192 * 1600}),
    # the C * R and F * R loops wrap (dwconv forward and dx, scale-residual, GELU and its backward); head.out.weight is ONE plane
    # of a 4100-frame fp32 chain (264 tiles: no split)
    "R4100_F512": ({**SMALL, "intermediate_dim": 512}, 2, 2050,
                   {"head.out": (1, 4100), "pwconv1": (4, 932), "pwconv2": (4, 932), "embed": (5, 772)},
                   {"dwconv, scale-residual (C R)": 512 * 4100, "GELU (F R)": 512 * 4100}),
    # split planes at the preset widths; the per-block activation stride times 8 layers at R > 128
    "preset_R260": ({}, 4, 65, {"head.out": (1, 260), "pwconv1": (2, 100), "pwconv2": (2, 100), "embed": (3, 68)}, {}),
}
REQUESTED_ABOVE_RETURNED = {("R1100", "pwconv1"), ("R1100", "pwconv2")}

# MEASURED (profiles/vocos_train_parity.txt, "Above 128 frames per batch"): relative L2 to the float64 restatement, bar 9.22e-06
MEASURED = """
not measured yet: this file has not run on an MI355X.  On the CPU: torch fp32's own error is 8.9e-07 .. 1.0e-06 (audio),
1.1e-06 .. 1.7e-06 (worst parameter) and 1.1e-06 .. 1.3e-06 (d mel) at the seven shapes and does not grow with R; an emulated
k-ordered fp32 chain of head.out.weight over the restatement's operands is 2.0e-07 (129 terms), 6.2e-07 (1100), 1.1e-06 (4100)
from float64.
"""


def _bar():
    """4 x the largest fp32-torch-vs-float64 error either fixture records for any parameter gradient (err32: the rule of
    tests/test_gpu_vocos_training.py for shapes the fixture lacks, over both files)."""
    worst = 0.0
    for fname, cases in (("vocos_grads.npz", R.CASES), ("vocos_grads_frames.npz", R.FRAME_CASES)):
        g = np.load(os.path.join(ROOT, "tests", "golden", fname))
        worst = max([worst] + [float(g[n + "/err32"].max()) for n in cases])
    return 4 * worst


def _wgrads(cfg):
    """name -> (Cin, Cout) of the weight gradients st_vocos_train_backward launches (pwconv1 / pwconv2 once per block)."""
    return {"head.out": (cfg.dim, cfg.n_fft + 2), "pwconv1": (cfg.dim, cfg.intermediate_dim), "pwconv2": (cfg.intermediate_dim, cfg.dim),
            "embed": (7 * cfg.input_channels, cfg.dim)}


@functools.lru_cache(maxsize=None)
def _inputs(case):
    fields, B, T, _, _ = CASES[case]
    cfg = vo.vocos_config(**fields)
    return cfg, vo.make_vocos_state_dict(WSEED, cfg), vo.make_mel(B, T, MSEED, M=cfg.input_channels), R.loss_weights((B, T * cfg.hop_length), WSEED)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """The float64 restatement, once per shape: (audio, {name: grad}, d mel, smallest |log-magnitude - ln 100|, clipped bins)."""
    cfg, sd, mel, W = _inputs(case)
    audio, kept = R.forward(sd, mel, cfg)
    G, dmel = R.backward(sd, kept, W.astype(np.float64), cfg)
    a = kept["o"][..., :cfg.n_fft // 2 + 1]
    out = (audio, G, dmel, float(np.abs(a - np.log(100.0)).min()), int((np.exp(a) > 100.0).sum()))
    for v in (audio, dmel, *G.values()):
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _native(case):
    """One native forward and backward per shape: (module, audio, {name: grad}, d mel)."""
    cfg, sd, mel, W = _inputs(case)
    mod = _module(cfg, sd)
    _, audio, grads, dmel = _run(mod, mel, _linear_loss(W))
    return mod, audio, grads, dmel


def _torch_fp32_errors(case):
    """torch fp32's own error at this shape: the same forward in torch ops under CPU autograd against the restatement."""
    cfg, sd, mel, W = _inputs(case)
    ref_audio, G, ref_dmel, _, _ = _reference(case)
    p = {k: torch.from_numpy(v).requires_grad_(k != "head.istft.window") for k, v in sd.items()}
    m = torch.from_numpy(mel).requires_grad_(True)
    audio = R.torch_vocos(p, m, cfg.num_layers)
    (audio * torch.from_numpy(W)).sum().backward()
    return (_rel_l2(audio.detach().numpy(), ref_audio), {n: _rel_l2(p[n].grad.numpy(), G[n]) for n in G}, _rel_l2(m.grad.numpy(), ref_dmel))


def _assert_paths(case):
    """Host-side: the case reaches the paths it is listed for (sw.wgrad_split is the Python port of fp32_tile.h's rule)."""
    fields, B, T, planes, wraps = CASES[case]
    cfg = vo.vocos_config(**fields)
    frames = B * T
    got = {}
    for name, (cin, cout) in _wgrads(cfg).items():
        tiles, want, fs, ret, capped = sw.wgrad_split(frames, cin, cout)
        got[name] = (ret, frames - (ret - 1) * fs)
        assert not capped and (ret < want) == ((case, name) in REQUESTED_ABOVE_RETURNED), (case, name, want, ret)
    assert got == planes, (case, got)
    assert max(p for p, _ in planes.values()) > 1 and planes["head.out"][0] == 1
    if case != "R129":
        assert frames > 256              # lane 0 of the 256-lane per-channel reductions adds a second frame
    for what, n in wraps.items():
        assert n > WRAP, (case, what, n)
    if "im2col (7 M R)" in wraps:
        assert wraps["im2col (7 M R)"] == 7 * cfg.input_channels * frames
    if "GELU (F R)" in wraps:
        assert wraps["GELU (F R)"] == cfg.intermediate_dim * frames and wraps["dwconv, scale-residual (C R)"] == cfg.dim * frames
    print(f"{case}: R = {B} x {T} = {frames}; planes x last-plane frames: " + ", ".join(f"{k} {p} x {l}" for k, (p, l) in got.items())
          + ("; loops that wrap: " + ", ".join(f"{k} = {n}" for k, n in wraps.items()) if wraps else ""))


@pytest.mark.parametrize("case", list(CASES))
def test_gradients_match_the_float64_restatement_above_128_frames(case):
    _assert_paths(case)
    bar = _bar()
    ref_audio, G, ref_dmel, clip_dist, clipped = _reference(case)
    # no log-magnitude sits within fp32 rounding of the clip, where the two precisions could disagree about the branch
    print(f"{case}: {clipped} clipped bins, nearest log-magnitude {clip_dist:.1e} from ln 100")
    assert clip_dist > 1e-4
    _, audio, grads, dmel = _native(case)
    assert sorted(grads) == sorted(G) and audio.shape == ref_audio.shape and dmel.shape == ref_dmel.shape
    ta, tg, td = _torch_fp32_errors(case)
    errs = {n: _rel_l2(grads[n], G[n]) for n in G}
    worst = max(errs, key=errs.get)
    ea, de = _rel_l2(audio, ref_audio), _rel_l2(dmel, ref_dmel)
    print(f"{case}: audio {ea:.2e} [torch fp32 {ta:.2e}], worst parameter {worst} {errs[worst]:.2e} [torch fp32 {tg[worst]:.2e}, its worst "
          f"{max(tg.values()):.2e}], head.out.weight {errs['head.out.weight']:.2e} [{tg['head.out.weight']:.2e}], d mel {de:.2e} "
          f"[torch fp32 {td:.2e}] (bar {bar:.2e})")
    assert np.isfinite(audio).all() and np.isfinite(dmel).all()
    assert ea <= bar and de <= bar
    for n, e in errs.items():
        assert np.isfinite(grads[n]).all() and e <= bar, (n, e)


def test_split_k_shapes_are_all_covered():
    """Which situations of the split rule, and of the flattened items against its frame ranges, the cases above put through
    launch_sd_wgrad."""
    seen = {}
    for case, (fields, B, T, _, _) in CASES.items():
        cfg = vo.vocos_config(**fields)
        frames = B * T
        for name, (cin, cout) in _wgrads(cfg).items():
            tiles, want, fs, ret, capped = sw.wgrad_split(frames, cin, cout)
            last = frames - (ret - 1) * fs
            bounds = range(fs, frames, fs)
            chunks = [(f0, min(f0 + 32, lo + fs, frames) - 1) for lo in range(0, ret * fs, fs) for f0 in range(lo, min(lo + fs, frames), 32)]
            shapes = {"one plane with at least 256 tiles": ret == 1 and tiles >= 256,
                      "several planes": ret > 1,
                      "fewer planes returned than requested": ret < want,
                      "a last plane that is no multiple of the 32-frame chunk": ret > 1 and last % 32 != 0,
                      "a last plane that ends in a one-frame chunk": ret > 1 and last % 32 == 1,
                      "a last plane of exactly one chunk": ret > 1 and last == 32,
                      "several planes over more than 16 column tiles": ret > 1 and cin > 1024,
                      "an item that straddles a plane boundary": ret > 1 and any(b % T != 0 for b in bounds),
                      "a chunk that straddles an item boundary": any(a // T != b // T for a, b in chunks)}
            assert not capped
            for k, hit in shapes.items():
                seen.setdefault(k, [])
                if hit:
                    seen[k].append(f"{case}/{name} ({frames} frames, {tiles} tiles: {want} requested, {ret} x {fs})")
    for k, v in seen.items():
        print(f"{k}: {len(v)} weight gradients, e.g. {(v or ['-'])[0]}")
    for k, v in seen.items():
        assert v, k


@pytest.mark.parametrize("name", list(R.FRAME_CASES))
def test_gradients_match_the_reference_module(name):
    """Against the REAL module's float64 gradients (vocos_grads_frames.npz), on the fixture's stored elements: per tensor, and
    for the audio and d mel, 4 x the fp32 reference module's own error of that tensor."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "vocos_grads_frames.npz"))
    fields, B, T, wseed, mseed, _ = R.FRAME_CASES[name]
    assert (fields, B, T) == CASES[name][:3] and (wseed, mseed) == (WSEED, MSEED)        # the run of _native is the fixture's case
    _, audio, grads, dmel = _native(name)
    names = list(gold[name + "/names"])
    assert sorted(grads) == names
    rows = []
    for i, n in enumerate(names):
        rows.append((n, _rel_l2(R.stored_elements(i, grads[n], wseed), gold[f"{name}/grad/{n}"]), float(gold[name + "/err32"][i])))
    rows.append(("audio", _rel_l2(R.sampled(audio, wseed, 1), gold[name + "/audio64"]), float(gold[name + "/audio_err32"])))
    rows.append(("d mel", _rel_l2(R.sampled(dmel, wseed, 0), gold[name + "/dmel64"]), float(gold[name + "/dmel_err32"])))
    print(f"{name}: relative L2 to the real module's float64 gradients (bar: 4 x torch fp32's own)")
    for n, err, own in rows:
        print(f"  {n:42s} native {err:.2e}  torch fp32 {own:.2e}  ratio {err / own:5.2f}")
    worst = max(rows[:-2], key=lambda r: r[1] / r[2])
    print(f"{name}: worst parameter ratio {worst[1] / worst[2]:.2f} ({worst[0]}), audio ratio {rows[-2][1] / rows[-2][2]:.2f}, "
          f"d mel ratio {rows[-1][1] / rows[-1][2]:.2f} (bar 4)")
    for n, err, own in rows:
        assert err <= 4 * own, (n, err, own)


def test_two_runs_are_bitwise_equal_and_items_do_not_mix_at_split_shapes():
    """R1100: 7 planes for the pwconvs, 5 for embed.  Two runs are bitwise equal; items 7 and 24 alone (their frames then sit at
    other tile, chunk and plane offsets than inside the batch) give their rows of the batch's audio and d mel bit for bit; the
    batch's parameter gradients are the sum of the 25 items' gradients within the bar."""
    case, bar = "R1100", _bar()
    cfg, sd, mel, W = _inputs(case)
    B = mel.shape[0]
    mod, a1, g1, d1 = _native(case)
    _, a2, g2, d2 = _run(mod, mel, _linear_loss(W))
    assert np.array_equal(a1, a2) and np.array_equal(d1, d2)
    for n in g1:
        assert np.array_equal(g1[n], g2[n]), n
    total = {n: np.zeros_like(v) for n, v in g1.items()}
    for b in range(B):
        _, ab, gb, db = _run(mod, mel[b:b + 1], _linear_loss(W[b:b + 1]))
        if b in (7, 24):
            assert np.array_equal(ab[0], a1[b]) and np.array_equal(db[0], d1[b]), b
        for n in gb:
            total[n] += gb[n]
    errs = {n: _rel_l2(g1[n], total[n]) for n in g1}
    worst = max(errs, key=errs.get)
    print(f"{case}: batch vs sum of the {B} items: worst {worst} {errs[worst]:.2e} (bar {bar:.2e})")
    assert errs[worst] <= bar


def test_shape_limits_of_the_c_abi_return_before_any_launch():
    """vt_check_shape (engine_vocos_train.cpp): more than 65535 items, and B * T times the widest row at or above 2^31, are
    ST_ERR_INVALID before anything is launched or allocated: the audio buffer keeps its sentinel, st_last_error names the limit."""
    from stabletts_amd import _lib
    cfg = vo.vocos_config(**SMALL)
    mod = _module(cfg, vo.make_vocos_state_dict(71, cfg))
    mel = torch.from_numpy(vo.make_mel(1, 2, 72, M=64)).cuda().requires_grad_(True)
    mod(mel)                                                         # binds the parameters; the engine is ready
    eng, lib = mod.engine(), _lib.load()
    x = mel.detach().contiguous()
    audio = torch.full((2 * 512,), 7.0, device="cuda")
    widest = max(7 * cfg.input_channels, cfg.intermediate_dim, 2 * 1152, cfg.n_fft)      # the head rows: two planes of 1152
    T_big = -(-(1 << 31) // widest)                                  # the smallest T with T * widest >= 2^31
    assert (T_big - 1) * widest < (1 << 31) <= T_big * widest and 65536 * widest < (1 << 31)
    for B, T, word in ((65536, 1, b"65535 items"), (1, T_big, b"B*T too large")):
        assert lib.st_vocos_train_forward(eng.handle, x.data_ptr(), audio.data_ptr(), B, T, None) == _lib.ST_ERR_INVALID, (B, T)
        assert word in lib.st_last_error(eng.handle), lib.st_last_error(eng.handle)
    torch.cuda.synchronize()
    assert torch.all(audio == 7.0)
    # the engine still works
    assert lib.st_vocos_train_forward(eng.handle, x.data_ptr(), audio.data_ptr(), 1, 2, None) == _lib.ST_OK
    torch.cuda.synchronize()
    assert torch.isfinite(audio).all() and not torch.any(audio == 7.0)
