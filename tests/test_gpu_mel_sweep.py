"""The spectrogram front end (audio_kernels.hip, audio_fft.h, engine_audio.cpp) on a real MI355X off the hop = n_fft / 4 lattice
of test_gpu_mel.py and test_gpu_mel_backward.py: forward and VJP of the log-mel and the linear module against float64
(tests/mel_restatement.py, tests/mel_vjp_restatement.py) at the cases of tests/mel_checks.py -- hop 1, hop = n_fft, odd hops,
pad 0, pad > hop, pad = n_fft - 1, an unread tail, n_mels = 2 n_fft -- with an asymmetric window whose ends are not zero; filter
banks the slaney construction never makes; the n_mels <= 2 n_fft limit of the backward; independence of batch items and
non-finite samples; ragged launches at small tiles, the growth of the utterance-table slots and the wrap of their ring.

Bar (tests/mel_checks.py): 4 x torch fp32's own distance from float64 on the same case and metric, pooled over a case's family
where its own yardstick is too small a sample; every error is printed beside its bar, test_sweep_summary prints the largest
ratio and the pooled cases (profiles/mel_sweep_parity.txt; measured: 251 comparisons, largest ratio 3.80, none pooled).  Run with
``-m gpu``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import mel_checks as mc
from tests import mel_restatement as mr
from tests import mel_vjp_restatement as mv

pytestmark = [pytest.mark.gpu, pytest.mark.grad]
REPORT = mc.Report()
LOG_FLOOR = float(np.log(1e-5))
ULP_AT_LOG_FLOOR = 2.0 ** -20                  # fp32 spacing in [8, 16)


def _modules(cfg, win, fb=None):
    """The trainable log-mel and linear modules of a configuration with `win` (and `fb`) loaded over the built buffers."""
    from stabletts_amd.audio_train import LinearSpectrogram, LogMelSpectrogram
    n_fft, hop, pad, n_mels = cfg
    lm = LogMelSpectrogram(mc.SR, n_fft, n_fft, hop, 0.0, None, pad, n_mels, False, "reflect", "slaney")
    lin = LinearSpectrogram(n_fft, n_fft, hop, pad, False, "reflect")
    sd = {"spectrogram.window": torch.from_numpy(win)}
    if fb is not None:
        sd["mel_scale.fb"] = torch.from_numpy(fb)
    lm.load_state_dict(sd, strict=False)
    lin.load_state_dict({"window": torch.from_numpy(win)})
    return lm.cuda(), lin.cuda()


def _native(module, wave, g):
    """(y, dx) of the native module in float32 numpy."""
    x = torch.from_numpy(wave).cuda().requires_grad_(True)
    y = module(x)
    y.backward(torch.from_numpy(g).cuda())
    return y.detach().cpu().numpy(), x.grad.cpu().numpy()


def _against_float64(name, module, kind, wave, r, pooled):
    """Forward and VJP of one module on one case against reference()'s entry r; `pooled(which)` gives the family's yardstick."""
    y, dx = _native(module, wave, r["g"])
    assert r["zeroed"] <= 1e-3 * r["g"].size, (name, r["zeroed"])
    assert y.shape == r["y"].shape and dx.shape == wave.shape and y.dtype == dx.dtype == np.float32
    assert np.isfinite(y).all() and np.isfinite(dx).all(), name
    ok = REPORT.held(f"{name} {kind}", mc.METRIC[kind](y, r["y"]), r["yard_y"], lambda: pooled("yard_y"))
    ok &= REPORT.held(f"{name} {kind} dx", mc.rel_max(dx, r["dx"]), r["yard_dx"], lambda: pooled("yard_dx"))
    return ok, y, dx


# ---- 1. the shape sweep ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.SWEEP, ids=mc.case_id)
def test_sweep_forward_and_vjp_match_float64(case):
    cfg, T, L, _ = case
    n_fft, hop, pad, n_mels = cfg
    wave, win, fb = mc.sweep_inputs(case)
    ref = mc.sweep_reference(case)
    lm, lin = _modules(cfg, win, fb)
    ok = True
    for kind, module, rows in (("log-mel", lm, n_mels), ("linear", lin, n_fft // 2 + 1)):
        good, y, dx = _against_float64(mc.case_id(case), module, kind, wave, ref[kind], lambda which: mc.pooled_yardstick(case, kind, which))
        ok &= good
        assert y.shape == (2, rows, T)
        if (n_fft, hop, pad) == (128, 100, 3):              # 96 samples that no frame reads, directly or by the right reflection
            assert np.all(dx[:, L - 96:] == 0.0) and np.all(ref[kind]["dx"][:, L - 96:] == 0.0) and np.all(dx[:, L - 97] != 0.0)
    assert ok, REPORT.fails


# ---- 2. filter banks the slaney construction never makes -------------------------------------------------------------------
BANK_CONFIGS = [(256, 64, 96, 40), (64, 7, 50, 10)]
BANK_NAMES = ["dense", "two_lobes", "column3_zero", "edge_rows_zero"]


def _bank_inputs(cfg):
    n_fft, hop, pad, n_mels = cfg
    L = mc.length_for(mc.tile(n_fft)[1] + 1, n_fft, hop, pad)
    return mc.waves(2, L, 31 + n_fft), mc.window(n_fft), mc.banks(n_fft, n_mels, 41 + n_fft)


@functools.lru_cache(maxsize=None)
def _bank_reference(cfg, name):
    wave, win, banks = _bank_inputs(cfg)
    return mc.reference(wave, win, banks[name], cfg[0], cfg[1], cfg[2], 51 + cfg[0] + BANK_NAMES.index(name))["log-mel"]


@pytest.mark.parametrize("name", BANK_NAMES)
@pytest.mark.parametrize("cfg", BANK_CONFIGS, ids=str)
def test_loaded_filter_banks_forward_and_vjp(cfg, name):
    n_fft, hop, pad, n_mels = cfg
    wave, win, banks = _bank_inputs(cfg)
    fb, bins = banks[name], n_fft // 2 + 1
    if name == "dense":
        assert (fb > 0).all()
    if name == "two_lobes":                                  # every filter: nonzero, zeros, nonzero inside its bin range
        for m in range(n_mels):
            nz = np.nonzero(fb[:, m])[0]
            assert len(nz) >= 4 and (fb[nz[0]:nz[-1] + 1, m] == 0).any()
    if name == "edge_rows_zero":
        assert not fb[0].any() and not fb[bins - 1].any() and fb[1].any() and fb[bins - 2].any()
    r = _bank_reference(cfg, name)
    lm, _ = _modules(cfg, win, fb)
    ok, y, dx = _against_float64(f"bank {name} {cfg}", lm, "log-mel", wave, r,
                                 lambda which: max(_bank_reference(cfg, n)[which] for n in BANK_NAMES))
    if name == "column3_zero":
        assert not fb[:, 3].any()
        assert np.all(y[:, 3] == y[0, 3, 0]) and abs(float(y[0, 3, 0]) - LOG_FLOOR) <= 3 * ULP_AT_LOG_FLOOR      # logf: 3 ulp (OpenCL)
        g0 = r["g"].copy()
        g0[:, 3] = 0.0
        assert r["g"][:, 3].any()
        _, dx0 = _native(lm, wave, g0)
        assert np.array_equal(dx, dx0)                       # the empty filter is in no bin's range: its g never enters
    assert ok, REPORT.fails


def test_backward_limit_at_n_mels_twice_n_fft():
    """n_fft = 32: 64 mels of a dense bank fill the two FFT buffers with dmel to the last float; 65 run forward and are refused
    backward (ST_ERR_UNSUPPORTED), before any launch."""
    from stabletts_amd import _lib
    n_fft, hop, pad = 32, 8, 12
    L = mc.length_for(65, n_fft, hop, pad)
    wave, win = mc.waves(2, L, 61), mc.window(n_fft)
    rng = np.random.Generator(np.random.PCG64(62))
    fb65 = (rng.uniform(0.0, 1.0, (17, 65)) / 17).astype(np.float32)
    ok = True
    for n_mels in (64, 65):
        fb = np.ascontiguousarray(fb65[:, :n_mels])
        r = mc.reference(wave, win, fb, n_fft, hop, pad, 63)["log-mel"]
        lm, _ = _modules((n_fft, hop, pad, n_mels), win, fb)
        if n_mels == 64:
            ok &= _against_float64("dense 64 mels at n_fft 32", lm, "log-mel", wave, r, lambda which: r[which])[0]
            continue
        x = torch.from_numpy(wave).cuda().requires_grad_(True)
        y = lm(x)
        assert y.shape == (2, 65, 65) and torch.isfinite(y).all()
        ok &= REPORT.held("dense 65 mels at n_fft 32 log-mel", mc.abs_max(y.detach().cpu().numpy(), r["y"]), r["yard_y"])
        with pytest.raises(_lib.NativeError) as ei:
            y.backward(torch.from_numpy(r["g"]).cuda())
        assert ei.value.code == _lib.ST_ERR_UNSUPPORTED and x.grad is None
        eng, lib = lm._engine(), _lib.load()
        w = torch.from_numpy(wave).cuda()
        go = torch.from_numpy(r["g"]).cuda()
        gx = torch.full((2, L), 7.0, device="cuda")
        ws = torch.empty(eng.mel_backward_workspace_bytes(2, L), dtype=torch.uint8, device="cuda")
        assert lib.st_mel_backward(eng.handle, w.data_ptr(), go.data_ptr(), 2, L, _lib.ST_MEL_LOG, gx.data_ptr(), ws.data_ptr(),
                                   None) == _lib.ST_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert torch.all(gx == 7.0)
    assert ok, REPORT.fails


# ---- 3. independence and non-finite input ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(64, 7, 50, 10), (2048, 300, 1000, 320)], ids=str)
def test_gradient_of_an_item_is_that_item_alone_bitwise(cfg):
    n_fft, hop, pad, n_mels = cfg
    T = mc.tile(n_fft)[1] + 1
    L = mc.length_for(T, n_fft, hop, pad)
    wave, other = mc.waves(3, L, 71 + n_fft), mc.waves(3, L, 72 + n_fft)
    lm, lin = _modules(cfg, mc.window(n_fft))
    rng = np.random.Generator(np.random.PCG64(73))
    for module, rows in ((lm, n_mels), (lin, n_fft // 2 + 1)):
        g, g2 = (rng.standard_normal((3, rows, T)).astype(np.float32) for _ in range(2))
        y, dx = _native(module, wave, g)
        assert np.abs(dx).min(1).max() > 0
        for b in range(3):
            yb, dxb = _native(module, wave[b:b + 1], g[b:b + 1])
            assert np.array_equal(yb[0], y[b]) and np.array_equal(dxb[0], dx[b]), b
        w2, gg = wave.copy(), g.copy()                       # another item's wave, then its g: items 0 and 2 do not move
        w2[1] = other[1]
        _, dxw = _native(module, w2, g)
        gg[1] = g2[1]
        _, dxg = _native(module, wave, gg)
        for b in (0, 2):
            assert np.array_equal(dxw[b], dx[b]) and np.array_equal(dxg[b], dx[b]), b
        assert not np.array_equal(dxw[1], dx[1]) and not np.array_equal(dxg[1], dx[1])


@pytest.mark.parametrize("cfg", [(32, 8, 12, 5), (512, 129, 200, 80)], ids=str)
def test_a_non_finite_sample_reaches_exactly_the_frames_that_read_it(cfg):
    """One NaN, then one +inf, at sample s of item 1 of 3, s next to the left edge (read directly and by the left reflection) and
    next to the right edge (by the right reflection): the frames whose padded window reads s (mc.readers: the index map) are NaN in
    every row, as in torch's forward; every other frame and item is bitwise the clean run's.  The magnitude of a +inf sample is
    +inf where the transform has no cancellation (torch, too, gives +inf bins there), so the linear module is held to NaN or +inf
    at +inf; neither bank has an empty filter (which reads no bin)."""
    n_fft, hop, pad, n_mels = cfg
    T = 2 * mc.tile(n_fft)[1] + 1
    L = mc.length_for(T, n_fft, hop, pad)
    wave, win, fb = mc.waves(3, L, 81 + n_fft), mc.window(n_fft), mc.slaney(n_fft, n_mels)
    assert (fb != 0).any(0).all()
    lm, lin = _modules(cfg, win)
    x = torch.from_numpy(wave).cuda()
    clean = {m: m(x) for m in (lm, lin)}
    for s in (3, L - 2):
        hit = mc.readers(s, L, T, n_fft, hop, pad)
        rest = np.setdiff1d(np.arange(T), hit)
        assert 0 < len(hit) < T and (s != 3 or 0 in hit) and (s != L - 2 or T - 1 in hit)
        for bad in (float("nan"), float("inf")):
            wb = wave.copy()
            wb[1, s] = bad
            yt = mv.torch_forward(torch.from_numpy(wb), torch.from_numpy(win), torch.from_numpy(fb), n_fft, hop, pad)
            assert torch.isnan(yt[1][:, hit]).all() and torch.isfinite(yt[1][:, rest]).all()
            xb = torch.from_numpy(wb).cuda()
            for m in (lm, lin):
                y = m(xb)
                broken = y[1][:, hit]
                nan_ok = torch.isnan(broken) if (m is lm or bad != bad) else (torch.isnan(broken) | (broken == float("inf")))
                print(f"{cfg} s={s} {bad} {'log-mel' if m is lm else 'linear'}: {len(hit)} frames read it; NaN {int(torch.isnan(broken).sum())}, "
                      f"+inf {int((broken == float('inf')).sum())} of {broken.numel()} entries")
                assert nan_ok.all(), (s, bad)
                assert torch.equal(y[1][:, rest], clean[m][1][:, rest]) and torch.equal(y[0], clean[m][0]) and torch.equal(y[2], clean[m][2])


# ---- 4. ragged launches at small tiles, and the slots of the utterance tables ------------------------------------------------
def _ragged_waves(cfg, counts, seed):
    n_fft, hop, pad, _ = cfg
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = [mc.length_for(T, n_fft, hop, pad) for T in counts]
    return [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens]


@pytest.mark.parametrize("cfg", [(32, 8, 12, 5), (64, 7, 50, 10)], ids=str)
def test_ragged_launch_mixes_utterances_below_at_and_above_a_tile(cfg):
    """1 (or the fewest the configuration allows), 63, 64, 65, 128 and 129 frames in one launch; a tile is 64 frames at n_fft = 32
    and 32 at 64."""
    from stabletts_amd import _lib
    n_fft, hop, pad, n_mels = cfg
    win, fb = mc.window(n_fft), mc.slaney(n_fft, n_mels)
    lm, lin = _modules(cfg, win)
    np_waves = _ragged_waves(cfg, [1, 63, 64, 65, 128, 129], 91 + n_fft)
    counts = [mr.frames(len(w), n_fft, hop, pad) for w in np_waves]
    assert counts[1:] == [63, 64, 65, 128, 129] and counts[0] == mr.frames(max(pad + 1, n_fft - 2 * pad), n_fft, hop, pad)
    waves = [torch.from_numpy(w).cuda() for w in np_waves]
    ok = True
    for kind, module, rows in (("log-mel", lm, n_mels), ("linear", lin, n_fft // 2 + 1)):
        outs = module.forward_ragged(waves)
        alone = [module(w[None])[0] for w in waves]
        refs = [mc.reference(w[None], win, fb, n_fft, hop, pad, 0)[kind] for w in np_waves]
        for b, (o, a, r) in enumerate(zip(outs, alone, refs)):
            assert o.shape == (rows, counts[b]) and torch.equal(o, a), b
            ok &= REPORT.held(f"ragged {cfg} utterance {b} ({counts[b]} frames) {kind}", mc.METRIC[kind](o.cpu().numpy()[None], r["y"]),
                              r["yard_y"], lambda: max(q["yard_y"] for q in refs))
        for order in (list(range(5, -1, -1)), [2, 3, 4, 5, 0, 1]):                  # reversed, rotated
            again = module.forward_ragged([waves[i] for i in order])
            assert all(torch.equal(again[j], outs[i]) for j, i in enumerate(order)), order
        # the C ABI on a NaN-filled output with a guard tail: every element written, nothing beyond rows * frame_offsets[B]
        eng = module._engine()
        so, fo = [0], [0]
        for w, T in zip(np_waves, counts):
            so.append(so[-1] + len(w))
            fo.append(fo[-1] + T)
        out = torch.full((rows * fo[-1] + 4096,), float("nan"), device="cuda")
        eng.mel_forward_ragged(torch.cat(waves), so, fo, _lib.ST_MEL_LOG if module is lm else _lib.ST_MEL_LINEAR, out,
                               torch.cuda.current_stream().cuda_stream)
        assert not torch.isnan(out[:rows * fo[-1]]).any() and torch.isnan(out[rows * fo[-1]:]).all()
        assert all(torch.equal(out[rows * fo[b]:rows * fo[b + 1]].view(rows, counts[b]), outs[b]) for b in range(6))
    assert ok, REPORT.fails


def test_slot_capacity_grows_with_the_batch_and_stays():
    """The utterance-table slots hold 64 entries until a launch needs more (B + 1 > 64): B = 65, then 130, then 3 on the same
    module; LinearSpectrogram.forward takes the ragged entry point on every dense call."""
    cfg = (32, 8, 12, 5)
    lm, lin = _modules(cfg, mc.window(32))
    fresh_lm, fresh_lin = _modules(cfg, mc.window(32))                              # each row alone, on handles that never grew
    rng = np.random.Generator(np.random.PCG64(101))
    dense = torch.from_numpy((0.3 * rng.standard_normal((65, 43))).astype(np.float32)).cuda()
    full = lin(dense)                                                               # B = 65 through the dense call
    assert full.shape == (65, 17, 5)
    assert all(torch.equal(full[b], fresh_lin(dense[b:b + 1])[0]) for b in range(65))
    for B in (65, 130, 3):
        waves = [torch.from_numpy((0.3 * rng.standard_normal(40 + b % 7)).astype(np.float32)).cuda() for b in range(B)]
        for module, fresh in ((lm, fresh_lm), (lin, fresh_lin)):
            outs = module.forward_ragged(waves)
            assert len(outs) == B
            for b, (w, o) in enumerate(zip(waves, outs)):
                assert torch.equal(o, fresh(w[None])[0]), (B, b)


def test_twelve_ragged_calls_back_to_back_wrap_the_slot_ring():
    """Four slots, twelve calls on one module and one stream with no synchronisation between them, queued behind enough other work
    that the host runs ahead of the device: a slot refilled before its launch has read it gives a call another call's table.
    The twelve tables are permutations of one list of lengths, so any of them stays inside any call's buffers."""
    cfg = (32, 8, 12, 5)
    n_fft, hop, pad, n_mels = cfg
    lm, _ = _modules(cfg, mc.window(32))
    rng = np.random.Generator(np.random.PCG64(111))
    counts = [1, 63, 64, 65, 2, 5, 17, 33]
    orders = [tuple(rng.permutation(8)) for _ in range(12)]
    assert len(set(orders)) == 12
    calls = [[torch.from_numpy(w).cuda() for w in _ragged_waves(cfg, [counts[i] for i in order], 112 + c)] for c, order in enumerate(orders)]
    lm.forward_ragged(calls[0])                                                     # the handle, its tables and slots exist
    busy = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    for _ in range(24):
        busy = torch.mm(busy, busy).clamp_(-1.0, 1.0)
    results = [lm.forward_ragged(ws) for ws in calls]
    torch.cuda.synchronize()
    for c, (ws, outs) in enumerate(zip(calls, results)):
        for b, (w, o) in enumerate(zip(ws, outs)):
            assert o.shape == (n_mels, counts[orders[c][b]]) and torch.equal(o, lm(w[None])[0]), (c, b)


def test_sweep_summary():
    """Prints the largest ratio to a bar and the cases that needed a pooled yardstick, of the tests of this file that ran."""
    print(f"{len(REPORT.lines)} comparisons; largest ratio to its yardstick {REPORT.worst[0]:.2f} ({REPORT.worst[1]}; bar 4); "
          f"pooled yardstick needed by {len(REPORT.pooled)}: {REPORT.pooled}")
    assert not REPORT.fails
