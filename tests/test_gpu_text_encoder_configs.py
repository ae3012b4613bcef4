"""Text encoder configs, loss heads and vocabulary sizes other than the default (V = 401, M = 128, F = 1024, L = 3, G = 256)
against the fp64 oracle on a real MI355X.  Run with ``-m gpu``.  The oracle itself is pinned to the reference by
test_oracle_golden.py.

  case    V     M    F     L   G     why
  M80     401   80   1024  3   256   partial 128-wide proj tile; proj.bias followed by an alignment gap in the flat gradient buffer
  M100    401   100  1024  3   256   as M80 (100 -> 112 floats)
  M300    401   300  1024  3   256   Mp = 384 > C: proj's weight gradient with cout16 > 256
  M1      401   1    1024  3   256   the narrowest proj
  F128    401   128  128   3   256   two-kernel FFN (F % 256 != 0), 128-wide tiles, fallback weight gradients with cout16 = F
  F384    401   128  384   3   256   as F128, with several 128-wide column tiles
  F2304   401   128  2304  3   256   fused FFN off although F % 256 == 0 (F > 2048)
  G4      401   128  1024  3   4     adaLN_modulation.0 over a 4-wide k chunk, its gradient in bwd_block_linears
  G260    401   128  1024  3   260   a 256-wide and a partial 4-wide k chunk
  G1024   401   128  1024  3   1024  four full k chunks
  L1      401   128  1024  1   256   a single block: block 0 is also the last
  L5      401   128  1024  5   256   an odd depth other than 3
  L16     401   128  1024  16  256   the most blocks the handle accepts, in ONE backward part

Every case runs in f16; M100, F384, G260 and L1 in bf16 as well.  Shapes are decoder_checks': B = 3, T = 130, lengths
[130, 97, 41] (three 64-frame tiles and a partial chunk).  Gates (text_encoder_checks.py): x 3e-4 / 3e-3 and mu_x 3e-4 / 2e-3
(f16 / bf16) of max |ref| for the inference forward; 3e-3 / 2e-2 for the loss, d c and every gradient but the q / k
projections, 1e-2 / 1e-1 for those; each raised to 1.5x the oracle's own operand-rounding floor where that is higher.

Measured on an MI355X, native error next to its gate (of max |ref|; "q/k": the worst q / k projection, "other": the worst other
parameter gradient).  The rounding floor raised the forward gates (f16 x to 3.2e-4 .. 6.7e-4, bf16 x to 4.0e-3 .. 4.9e-3) and no
gradient gate; no case came near the q / k gate, so no case needed a gate above TOL_QK.

  case   dt    x        mu_x     loss     d c      other    (gate)  q/k      (gate)
  M80    f16   8.3e-05  5.2e-05  2.5e-05  5.0e-04  6.4e-04  3e-3    1.2e-03  1e-2
  M100   f16   8.6e-05  7.8e-05  4.8e-05  5.4e-04  6.6e-04  3e-3    1.6e-03  1e-2
  M300   f16   1.1e-04  5.0e-05  2.8e-05  6.0e-04  9.1e-04  3e-3    8.2e-04  1e-2
  M1     f16   8.8e-05  4.0e-05  6.1e-05  4.6e-04  6.0e-04  3e-3    1.4e-03  1e-2
  F128   f16   7.0e-05  5.2e-05  1.8e-05  8.0e-04  7.9e-04  3e-3    1.3e-03  1e-2
  F384   f16   7.7e-05  5.0e-05  1.3e-04  6.9e-04  7.9e-04  3e-3    1.6e-03  1e-2
  F2304  f16   7.8e-05  5.8e-05  1.1e-03  4.8e-04  6.7e-04  3e-3    1.9e-03  1e-2
  G4     f16   6.4e-05  3.8e-05  2.0e-04  3.3e-04  1.0e-03  3e-3    1.2e-03  1e-2
  G260   f16   5.1e-05  3.0e-05  1.3e-05  6.1e-04  8.6e-04  3e-3    1.2e-03  1e-2
  G1024  f16   3.6e-05  2.9e-05  6.3e-06  4.5e-04  8.3e-04  3e-3    2.0e-03  1e-2
  L1     f16   7.1e-05  4.4e-05  3.9e-05  6.3e-04  6.3e-04  3e-3    1.1e-03  1e-2
  L5     f16   9.2e-05  8.3e-05  4.7e-05  6.5e-04  6.9e-04  3e-3    1.3e-03  1e-2
  L16    f16   1.4e-04  1.3e-04  3.0e-05  5.2e-04  7.5e-04  3e-3    1.5e-03  1e-2
  M100   bf16  6.0e-04  4.7e-04  1.8e-04  3.9e-03  5.4e-03  2e-2    1.1e-02  1e-1
  F384   bf16  5.8e-04  4.4e-04  3.0e-04  4.8e-03  5.9e-03  2e-2    1.4e-02  1e-1
  G260   bf16  3.6e-04  2.6e-04  3.6e-06  4.3e-03  8.3e-03  2e-2    1.1e-02  1e-1
  L1     bf16  5.4e-04  3.1e-04  1.3e-05  5.2e-03  5.4e-03  2e-2    7.6e-03  1e-1

Loss heads (f16; default / M100): x only: other 6.6e-4 / 5.7e-4, q/k 1.1e-3 / 1.0e-3; mu_x only: other 7.5e-4 / 7.4e-4, q/k
1.5e-3 / 1.4e-3; the one-sided gradients summed against the two-sided: worst tensor 7.6e-4 / 9.0e-4 (gate 3e-3).  d emb.weight
(gate 3e-3): V = 1: 2.8e-4, 2: 2.8e-4, 1024: 2.6e-4, 1025: 1.7e-4, 2500: 2.8e-4, 1300 at 16896 rows: 2.5e-4.  The flat buffer
has 12 gap floats at M100 and none at the default config and G260; nothing outside the slices was written.

The loss-head tests run the default config and M100 with a loss from x only (st_text_encoder_train_backward's grad_mu == NULL
branch), from mu_x only (grad_x == NULL) and from both, at the same inputs and gates.  The vocabulary tests run L = 1 at
V = 1, 2, 1024, 1025, 2500 (B = 2, T = 300) and V = 1300 at 16896 rows (66 row chunks): emb_scan_kernel's second and third
pass, emb_colscan_kernel's exit at V % 4 = 0, 1, 2 and its second 64-chunk step, emb_piece_kernel's search over runs of ids
without rows.  At V = 1 and V = 2 every id is used (token 0 and the clamped ids), so the "at least half of the ids occur in no
valid row" property is asserted from V = 1024 on.  The bounds test is decoder_checks.check_backward_bounds for this kind
(the text encoder's backward is one part).
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle.make_golden_text_encoder import text_inputs
from oracle.weights import TextEncoderConfig
from text_encoder_checks import (B, LENGTHS, T, TOL, check_backward_bounds, check_forward, check_gradients, embedding_gradient_reference,
                                 loss_weights, module, native_grads, reference, rel, rounding_floor)

pytestmark = pytest.mark.gpu

# name: (config changes from the default, seed)
CONFIGS = {
    "default": ({}, 30),
    "M80": (dict(out_channels=80), 31),
    "M100": (dict(out_channels=100), 32),
    "M300": (dict(out_channels=300), 33),
    "M1": (dict(out_channels=1), 34),
    "F128": (dict(filter_channels=128), 35),
    "F384": (dict(filter_channels=384), 36),
    "F2304": (dict(filter_channels=2304), 37),
    "G4": (dict(gin_channels=4), 38),
    "G260": (dict(gin_channels=260), 39),
    "G1024": (dict(gin_channels=1024), 40),
    "L1": (dict(n_layers=1), 41),
    "L5": (dict(n_layers=5), 42),
    "L16": (dict(n_layers=16), 43),
}
SWEEP = [n for n in CONFIGS if n != "default"]
BF16 = ["M100", "F384", "G260", "L1"]
CASES = [(n, "f16") for n in SWEEP] + [(n, "bf16") for n in BF16]
HEADS = ["default", "M100"]
BOUNDS = ["default", "M100", "G260"]


def _config(name):
    return TextEncoderConfig(**CONFIGS[name][0])


@functools.lru_cache(maxsize=None)
def _state_dict(name):
    return oracle.make_text_encoder_state_dict(900 + CONFIGS[name][1], _config(name))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    cf, s = _config(name), CONFIGS[name][1]
    tok, c, lens = text_inputs(B, T, LENGTHS, 100 + s, n_vocab=cf.n_vocab, gin=cf.gin_channels)
    w_mu, w_x = loss_weights(B, T, 100 + s, cf.out_channels, cf.hidden_channels)
    return tok, c, lens, w_mu, w_x


def _args(name, head="both"):
    tok, c, lens, w_mu, w_x = _inputs(name)
    return tok, c, lens, (w_mu if head != "x" else None), (w_x if head != "mu" else None)


@functools.lru_cache(maxsize=None)
def _ref(name, head):
    """The fp64 oracle on the case's inputs (CPU): forward, loss, d c and every gradient."""
    return reference(_state_dict(name), *_args(name, head))


@functools.lru_cache(maxsize=None)
def _floor(name, dt, head):
    return rounding_floor(_ref(name, head), _state_dict(name), *_args(name, head), dt)


def _module(name, dt="f16"):
    return module(_config(name), _state_dict(name), dt)


@pytest.mark.parametrize("name,dt", CASES)
def test_inference_forward_vs_oracle(name, dt):
    tok, c, lens, _, _ = _inputs(name)
    check_forward(name, _module(name, dt), tok, c, lens, _ref(name, "both"), _floor(name, dt, "both"), dt)


@pytest.mark.grad
@pytest.mark.parametrize("name,dt", CASES)
def test_loss_and_every_gradient_vs_oracle_autograd(name, dt):
    got = native_grads(_module(name, dt), *_args(name))
    check_gradients(name, got, _ref(name, "both"), _floor(name, dt, "both"), dt)


# ---------------------------------------------------------------------------------------------------------------- loss heads
@functools.lru_cache(maxsize=None)
def _heads(name):
    """native_grads of ONE f16 module with the loss from both outputs, from x only and from mu_x only."""
    m = _module(name)
    return {h: native_grads(m, *_args(name, h)) for h in ("both", "x", "mu")}


@pytest.mark.grad
@pytest.mark.parametrize("name", HEADS)
def test_loss_from_x_only(name):
    """grad_mu is None: bwd_head_text scales from grad_x alone and zeroes d X and proj's gradients."""
    got = _heads(name)["x"]
    ref = _ref(name, "x")
    assert ref["grads"]["proj.weight"] is None and ref["grads"]["proj.bias"] is None
    check_gradients(f"{name} x only", got, ref, _floor(name, "f16", "x"), "f16")
    for n in ("proj.weight", "proj.bias"):
        assert got[2][n] is not None and torch.count_nonzero(got[2][n]) == 0, n


@pytest.mark.grad
@pytest.mark.parametrize("name", HEADS)
def test_loss_from_mu_x_only(name):
    """grad_x is None: only proj feeds the last block's gradient."""
    ref = _ref(name, "mu")
    assert all(g is not None for g in ref["grads"].values())
    check_gradients(f"{name} mu_x only", _heads(name)["mu"], ref, _floor(name, "f16", "mu"), "f16")


@pytest.mark.grad
@pytest.mark.parametrize("name", HEADS)
def test_one_sided_gradients_add_up_to_the_two_sided(name):
    """The backward is linear in the output gradients; the power-of-two rescaling differs between the three runs, so the sum holds
    within TOL per tensor and not bit for bit."""
    h = _heads(name)
    both, gx, gmu = h["both"], h["x"], h["mu"]
    err = {n: rel(gx[2][n].double() + gmu[2][n].double(), both[2][n]) for n in both[2]}
    ec = rel(gx[1].double() + gmu[1].double(), both[1])
    el = abs(gx[0] + gmu[0] - both[0]) / max(abs(both[0]), 1.0)
    worst = max((v, n) for n, v in err.items())
    print(f"[{name} f16] x-only + mu_x-only vs two-sided: loss {el:.2e}, d c {ec:.2e}, worst gradient {worst[0]:.2e} ({worst[1]}), gate {TOL['f16']:.0e}")
    assert el <= TOL["f16"] and ec <= TOL["f16"]
    bad = {n: v for n, v in err.items() if v > TOL["f16"]}
    assert not bad, bad


@pytest.mark.grad
@pytest.mark.parametrize("name", HEADS)
def test_c_without_grad_and_frozen_embedding_are_bit_identical(name):
    both = _heads(name)["both"]
    m = _module(name)
    loss, gc, g = native_grads(m, *_args(name), c_grad=False)
    assert gc is None and loss == both[0]
    for n in both[2]:
        assert torch.equal(g[n], both[2][n]), n
    m.emb.weight.requires_grad_(False)
    loss, gc, g = native_grads(m, *_args(name))
    assert m.emb.weight.grad is None and g["emb.weight"] is None
    assert loss == both[0] and torch.equal(gc, both[1])
    for n in both[2]:
        if n != "emb.weight":
            assert torch.equal(g[n], both[2][n]), n


# ---------------------------------------------------------------------------------------------------------------- vocabulary
def _vocab_ids(V, Bn, Tn, lengths, seed):
    """Ids with token 0 at every other position, the other positions drawn from a pool of fewer than V / 4 ids that holds the ids on
    both sides of every 1024 boundary, one id < 0 and one >= V (clamped to 0 and V - 1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    must = sorted({v for v in (0, 1023, 1024, 2047, 2048, V - 1) if v < V})
    pool = np.unique(np.concatenate([np.array(must), rng.integers(0, V, size=max(1, min(V // 4, 150)))]))
    tok = pool[rng.integers(0, len(pool), size=(Bn, Tn))].astype(np.int64)
    tok[:, 0::2] = 0
    short = int(np.argmin(lengths))                 # the required ids inside the shortest item's valid rows
    assert 2 * len(must) + 1 <= lengths[short]
    for j, v in enumerate(must):
        tok[short, 2 * j + 1] = v
    long_ = int(np.argmax(lengths))
    tok[long_, 5] = -7
    tok[long_, 7] = 10 ** 6
    return torch.from_numpy(tok), must


def _vocab_case(V, Bn, Tn, lengths, seed):
    cfg = TextEncoderConfig(n_vocab=V, n_layers=1)
    sd = oracle.make_text_encoder_state_dict(1700 + seed, cfg)
    tok, must = _vocab_ids(V, Bn, Tn, lengths, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    c = torch.from_numpy(rng.standard_normal((Bn, 256)).astype(np.float32))
    lens = torch.tensor(lengths)
    w_mu, w_x = loss_weights(Bn, Tn, seed)
    ref, used = embedding_gradient_reference(sd, tok, c, lens, w_mu, w_x)
    assert all(bool(used[v]) for v in must) and bool(used[V - 1]) and bool(used[0])
    if V >= 1024:
        assert 2 * int(used.sum()) <= V, "at least half of the ids must occur in no valid row"
    m = module(cfg, sd, "f16")
    r1 = native_grads(m, tok, c, lens, w_mu, w_x)
    r2 = native_grads(m, tok, c, lens, w_mu, w_x)
    assert r1[0] == r2[0] and torch.equal(r1[1], r2[1])
    assert all(torch.equal(r1[2][n], r2[2][n]) for n in r1[2]), "not bitwise repeatable"
    got = r1[2]["emb.weight"]
    e = rel(got, ref)
    print(f"[V={V} B={Bn} T={Tn}] {int(used.sum())} of {V} ids used; d emb.weight vs index_add of the oracle's d x0 {e:.2e} (gate {TOL['f16']:.0e})")
    assert e <= TOL["f16"]
    assert torch.count_nonzero(got[~used]) == 0
    assert all(float(got[v].abs().max()) > 0 for v in must)


@pytest.mark.grad
@pytest.mark.parametrize("V", [1, 2, 1024, 1025, 2500])
def test_embedding_gradient_vocabulary_sizes(V):
    """emb_scan_kernel's carry between 1024-id passes (V > 1024), emb_colscan_kernel's v >= V exit at V % 4 = 0, 1, 2,
    emb_piece_kernel's search over many ids without rows, and V = 1 where every row lands in one bucket."""
    _vocab_case(V, 2, 300, [300, 173], 50 + V % 7)


@pytest.mark.grad
def test_embedding_gradient_more_than_64_row_chunks():
    """V = 1300 at 66 x 256 = 16896 rows (66 chunks of 256 rows, ragged: chunks hold padded rows): emb_colscan_kernel's second
    64-chunk step together with emb_scan_kernel's second pass."""
    rng = np.random.Generator(np.random.PCG64(66))
    lengths = [256] + [int(v) for v in rng.integers(40, 257, size=65)]
    assert sum(1 for v in lengths if v < 256) >= 32
    _vocab_case(1300, 66, 256, lengths, 66)


# ---------------------------------------------------------------------------------------------------------------- bounds
@pytest.mark.grad
@pytest.mark.parametrize("name", BOUNDS)
def test_backward_stays_inside_the_gradient_slices(name, monkeypatch):
    """text_encoder_checks.check_backward_bounds: nothing outside the parameter slices of a caller-owned buffer changes, the slices
    equal the autograd gradients, and ST_TRAIN_SIDE=0 gives the same buffer, d c, x and mu_x bit for bit."""
    check_backward_bounds(name, lambda: _module(name), *_inputs(name), monkeypatch)
