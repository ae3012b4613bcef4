"""Native training path of the TextEncoder (st_text_encoder_train_forward / st_text_encoder_train_backward behind
stabletts_amd.text_encoder's autograd Function) on a real MI355X: gradients against the REAL reference module
(tests/golden/text_encoder_grads.npz, tools/make_golden_text_encoder_grads.py), against autograd through the fp32 oracle
(oracle.text_encoder_forward) at training size, the embedding gradient's determinism under token-0 skew, counter-based
dropout with the oracle run on the same masks, AdamW steps, the error path, train.py's loss chain with the native decoder and
a 2-rank DDP run.  Run with ``-m gpu``.

Gates: max |native - ref| / max |ref| per tensor, the decoder's training bars (tests/test_gpu_training.py, whose docstring
explains the looser conv_q / conv_k bars).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle.make_golden_text_encoder import text_inputs
from oracle.weights import TextEncoderConfig
from text_encoder_checks import TOL, TOL_QK, loss_weights as _loss_weights, oracle_grads as _oracle

pytestmark = [pytest.mark.gpu, pytest.mark.grad]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _tol(name, dt):
    return (TOL_QK if (".attn.conv_q." in name or ".attn.conv_k." in name) else TOL)[dt]


def _module(sd, dt, gin=256, train=False):
    from stabletts_amd.text_encoder import TextEncoder
    m = TextEncoder(401, 128, 256, 1024, 4, 3, 3, 0.1, gin, operand_dtype=dt)
    m.load_state_dict(sd)
    m = m.cuda()
    return m.train() if train else m.eval()


def _native(m, tok, c, lens, w_mu, w_x):
    """loss, d c and every parameter gradient of the native module."""
    m.zero_grad(set_to_none=True)
    cc = c.cuda().clone().requires_grad_(True)
    x, mu_x, mask = m(tok.cuda(), cc, lens.cuda())
    assert not mask.requires_grad
    loss = (mu_x * w_mu.cuda()).sum() + (x * w_x.cuda()).sum()
    loss.backward()
    return float(loss.detach()), cc.grad.cpu(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}


def _check(dt, got, ref, label):
    lg, gcg, gg = got
    lr, gcr, gr = ref
    worst = {n: _rel(gg[n].numpy(), gr[n].numpy()) for n in gr}
    bad = {n: v for n, v in worst.items() if v > _tol(n, dt)}
    ec = _rel(gcg.numpy(), gcr.numpy())
    print(f"[{label} {dt}] loss {lg:.6g} / {lr:.6g}, d c {ec:.2e}, worst non-q/k {max(v for n, v in worst.items() if _tol(n, dt) == TOL[dt]):.2e}"
          f", q/k {max(v for n, v in worst.items() if _tol(n, dt) != TOL[dt]):.2e}")
    assert abs(lg - lr) <= TOL[dt] * max(abs(lr), 1.0)
    assert ec <= TOL[dt]
    assert not bad, bad


@pytest.fixture(scope="module")
def enc_sd():
    return oracle.make_text_encoder_state_dict(2468)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("case", ["small", "edge"])
def test_gradients_match_reference_fixture(enc_sd, dt, case):
    g = np.load(os.path.join(ROOT, "tests", "golden", "text_encoder_grads.npz"))
    tok, c, lens = (torch.from_numpy(g[f"{case}/{k}"]) for k in ("tokens", "c", "lengths"))
    B, T = tok.shape
    assert torch.equal(tok, text_inputs(B, T, lens.tolist(), {"small": 31, "edge": 32}[case])[0])
    w_mu, w_x = _loss_weights(B, T, {"small": 31, "edge": 32}[case])
    m = _module(enc_sd, dt)
    loss, gc, gp = _native(m, tok, c, lens, w_mu, w_x)
    ref_loss = g[f"{case}/loss"].item()      # (a sum of terms of both signs: gated like the gradients)
    assert abs(loss - ref_loss) <= TOL[dt] * abs(ref_loss)
    assert _rel(gc.numpy(), g[f"{case}/grad_c"]) <= TOL[dt]
    names, norms = [str(n) for n in g[f"{case}/norm_names"]], g[f"{case}/norms"]
    assert sorted(gp) == names
    bad = {n: (float(gp[n].double().norm()), r) for n, r in zip(names, norms) if abs(float(gp[n].double().norm()) - r) > _tol(n, dt) * r}
    assert not bad, bad
    for key in g.files:
        if key.startswith(f"{case}/full/"):
            n = key[len(f"{case}/full/"):]
            assert _rel(gp[n].numpy(), g[key]) <= _tol(n, dt), n
    ids = torch.from_numpy(g[f"{case}/emb_ids"])
    assert _rel(gp["emb.weight"][ids].numpy(), g[f"{case}/emb_rows"]) <= TOL[dt]
    unused = torch.ones(401, dtype=torch.bool); unused[ids] = False
    assert torch.count_nonzero(gp["emb.weight"][unused]) == 0


def _ragged(B, T, seed, lo=0.6):
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = [T] + [int(v) for v in rng.integers(max(1, int(lo * T)), T + 1, size=B - 1)]
    return lengths


@pytest.mark.parametrize("B,T,gin,weights", [(64, 300, 256, "seeded"), (2, 1000, 256, "seeded"), (1, 1, 256, "seeded"),
                                             (3, 77, 192, "seeded"), (4, 150, 256, "trained")])
def test_gradients_match_oracle_at_training_size(B, T, gin, weights):
    cfg = TextEncoderConfig(gin_channels=gin)
    sd = oracle.make_text_encoder_state_dict(77, cfg, ada_std=0.15 if weights == "trained" else 0.02)
    # "trained": adaLN weights of std 0.15 (gates and scales of O(1), as after training) instead of the near-identity 0.02.
    # (Scaling q / k up as well, for arg-max attention, moves the fp32 loss itself by 0.4 % when only q, k are rounded to 16 bits:
    # there the comparison has to be made at the native q, k, v, as test_gpu_training.py's trained-like test does.)
    lengths = _ragged(B, T, 5 + B) if T > 1 else [1] * B
    tok, c, lens = text_inputs(B, T, lengths, 40 + B, gin=gin)
    w_mu, w_x = _loss_weights(B, T, 40 + B)
    m = _module(sd, "f16", gin)
    _check("f16", _native(m, tok, c, lens, w_mu, w_x), _oracle(sd, tok, c, lens, w_mu, w_x), f"B={B} T={T} gin={gin} {weights}")


def test_embedding_gradient_skewed_deterministic_and_exact_zeros(enc_sd):
    B, T = 8, 257
    lengths = [257, 200, 131, 64, 63, 33, 2, 1]
    rng = np.random.Generator(np.random.PCG64(3))
    tok = torch.from_numpy(rng.integers(1, 60, size=(B, T)).astype(np.int64))      # ids 60..399 never occur
    tok[:, 0::2] = 0                                                               # token 0 at half the positions (intersperse)
    tok[0, 5] = -7; tok[1, 7] = 10 ** 6                                            # clamped to 0 and 400, as the forward reads them
    c = torch.from_numpy(rng.standard_normal((B, 256)).astype(np.float32))
    lens = torch.tensor(lengths)
    w_mu, w_x = _loss_weights(B, T, 3)
    m = _module(enc_sd, "f16")
    r1 = _native(m, tok, c, lens, w_mu, w_x)
    r2 = _native(m, tok, c, lens, w_mu, w_x)
    assert r1[0] == r2[0] and torch.equal(r1[1], r2[1])
    assert all(torch.equal(r1[2][n], r2[2][n]) for n in r1[2]), "not bitwise repeatable"
    # d emb = sqrt(C) * index_add of the oracle's d x0 (fp64) over the valid positions, at the clamped ids
    sd = {k: v.double() for k, v in enc_sd.items()}
    pr = {k: v.clone() for k, v in sd.items()}
    x0 = (torch.nn.functional.embedding(tok.clamp(0, 400), sd["emb.weight"]) * 16.0).transpose(1, 2).detach().requires_grad_(True)
    mask = (torch.arange(T)[None] < lens[:, None]).unsqueeze(1).double()
    x = x0
    for i in range(3):
        x = oracle.dit_conv_block(pr, f"encoder.{i}.", x, c.double(), mask)
    mu_x = torch.nn.functional.conv1d(x, pr["proj.weight"], pr["proj.bias"]) * mask
    ((mu_x * w_mu.double()).sum() + (x * w_x.double()).sum()).backward()
    dx0 = x0.grad.transpose(1, 2) * mask.transpose(1, 2)                           # (B, T, C), valid rows only
    ref = torch.zeros(401, 256, dtype=torch.float64).index_add_(0, tok.clamp(0, 400).reshape(-1), dx0.reshape(-1, 256)) * 16.0
    got = r1[2]["emb.weight"]
    print(f"[emb] d emb.weight vs fp64 index_add {_rel(got.numpy(), ref.numpy()):.2e}")
    assert _rel(got.numpy(), ref.numpy()) <= TOL["f16"]
    used = torch.zeros(401, dtype=torch.bool)
    for b in range(B):
        used[tok[b, :lengths[b]].clamp(0, 400)] = True
    assert torch.count_nonzero(got[~used]) == 0 and bool(used[400]) and int(used.sum()) < 100


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_dropout_matches_oracle_with_the_same_masks(enc_sd, dt):
    from oracle.estimator_oracle import layer_norm_c, mha, ffn
    from tests.test_gpu_training import _drop_attn, _drop_ffn
    B, T, p, F_, H = 2, 70, 0.1, 1024, 4
    tok, c, lens = text_inputs(B, T, [70, 45], 61)
    w_mu, w_x = _loss_weights(B, T, 61)
    m = _module(enc_sd, dt, train=True)

    def native(seed):
        torch.manual_seed(seed)
        return _native(m, tok, c, lens, w_mu, w_x)

    r1, r1b, r2 = native(123), native(123), native(124)
    assert r1[0] == r1b[0] and r1[0] != r2[0]
    torch.manual_seed(123)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    n_, t_, c_ = np.meshgrid(np.arange(B), np.arange(T), np.arange(F_), indexing="ij")
    idx = ((n_ * T + t_) * F_ + c_).astype(np.uint64)
    nn_, hh, qq, kk = np.meshgrid(np.arange(B), np.arange(H), np.arange(T), np.arange(T), indexing="ij")
    d_ffn = [torch.from_numpy(_drop_ffn(seed, 2 * i, p, idx)).permute(0, 2, 1).double() for i in range(3)]
    d_att = [torch.from_numpy(_drop_attn(seed, 2 * i + 1, p, ((nn_ * H + hh) * T + qq).astype(np.uint64), kk.astype(np.uint64))).double()
             for i in range(3)]
    mask = (torch.arange(T)[None] < lens[:, None]).unsqueeze(1).double()

    def fwd(pr, cc):      # dit_conv_block (oracle) with the dropout factors of the native forward
        x = torch.nn.functional.embedding(tok, pr["emb.weight"]) * 16.0
        x = x.transpose(1, 2)
        F = torch.nn.functional
        for i in range(3):
            pre = f"encoder.{i}."
            x = x * mask
            ada = F.linear(F.silu(cc), pr[pre + "adaLN_modulation.2.weight"], pr[pre + "adaLN_modulation.2.bias"])
            sh_a, sc_a, g_a, sh_m, sc_m, g_m = ada.unsqueeze(2).chunk(6, dim=1)
            h = layer_norm_c(x) * (1 + sc_a) + sh_a
            x = x + g_a * mha(pr, pre + "attn.", h, mask, drop=d_att[i]) * mask
            h = layer_norm_c(x) * (1 + sc_m) + sh_m
            x = x + g_m * ffn(pr, pre + "mlp.", h, mask, drop=d_ffn[i])
        return x, F.conv1d(x, pr["proj.weight"], pr["proj.bias"]) * mask

    _check(dt, r1, _oracle(enc_sd, tok, c, lens, w_mu, w_x, fwd=fwd), "dropout")


def test_adamw_trajectory_and_inference_after_steps(enc_sd):
    B, T = 4, 90
    tok, c, lens = text_inputs(B, T, [90, 71, 40, 13], 71)
    w_mu, w_x = _loss_weights(B, T, 71)
    m = _module(enc_sd, "f16")
    pr = {k: v.clone().requires_grad_(True) for k, v in enc_sd.items()}
    names = [n for n, _ in m.named_parameters()]
    opt_n = torch.optim.AdamW(m.parameters(), lr=1e-4)
    opt_o = torch.optim.AdamW([pr[n] for n in names], lr=1e-4)
    eng0 = m.engine()
    for step in range(5):
        ln, _, gn = _native(m, tok, c, lens, w_mu, w_x)
        if step == 0:
            bytes0 = eng0.device_bytes()      # (the training state is allocated by the first grad-enabled forward)
        opt_n.step()
        opt_o.zero_grad()
        x, mu_x, _ = oracle.text_encoder_forward(pr, tok, c, lens)
        lo = (mu_x * w_mu).sum() + (x * w_x).sum()
        lo.backward()
        if step == 0:
            kb0 = {n: (gn[n], pr[n].grad.clone(), pr[n.replace("conv_k", "conv_q")].grad.clone()) for n in names if n.endswith("attn.conv_k.bias")}
        opt_o.step()
        assert abs(ln - float(lo.detach())) <= 2e-3 * abs(float(lo.detach())), step
    assert m.engine() is eng0 and eng0.device_bytes() == bytes0       # re-packed in place: no new engine, no new buffers
    # The gate is the direction of every tensor's accumulated update (cosine, as the decoder's trajectory test): Adam normalises
    # each element's step to ~lr, so a per-element distance bound would hold whatever the gradients were.
    cos = {}
    for n, p in m.named_parameters():
        a, b, p0 = p.detach().cpu().double(), pr[n].detach().double(), enc_sd[n].double()
        da, db = (a - p0).reshape(-1), (b - p0).reshape(-1)
        cos[n] = float(da @ db / max(float(da.norm() * db.norm()), 1e-30))
    # conv_k.bias: a key bias adds the same q.b to every score of a query but for RoPE's rotation, so its gradient is tiny next to
    # the layer's other gradients and its Adam update mostly sign noise (update cosine ~0.8).  Its gate is the first step's
    # gradient instead: the native one within the q / k bar of the oracle's, measured against the size of conv_q.bias's gradient.
    kb = sorted(kb0)
    kerr = {n: float((kb0[n][0].double() - kb0[n][1].double()).abs().max() / kb0[n][2].abs().max()) for n in kb}
    print(f"[adamw] 5 steps: update cosine min {min(v for n, v in cos.items() if n not in kb):.5f}; conv_k.bias update cosine "
          f"{min(cos[n] for n in kb):.3f}, first-step gradient error {max(kerr.values()):.2e} of |d conv_q.bias|")
    assert min(v for n, v in cos.items() if n not in kb) >= 0.995, cos
    assert max(kerr.values()) <= TOL_QK["f16"], kerr
    fresh = _module({n: p.detach().cpu() for n, p in m.named_parameters()}, "f16")
    with torch.no_grad():
        a = m(tok.cuda(), c.cuda(), lens.cuda())
        b = fresh(tok.cuda(), c.cuda(), lens.cuda())
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_stale_backward_raises(enc_sd):
    B, T = 2, 40
    tok, c, lens = text_inputs(B, T, [40, 22], 81)
    m = _module(enc_sd, "f16")
    x1, mu1, _ = m(tok.cuda(), c.cuda(), lens.cuda())
    x2, mu2, _ = m(tok.cuda(), c.cuda(), lens.cuda())
    with pytest.raises(RuntimeError, match="activations are gone"):
        mu1.sum().backward()
    mu2.sum().backward()                     # the live forward still works
    assert m.emb.weight.grad is not None and torch.isfinite(m.emb.weight.grad).all()
    x3, mu3, _ = m(tok.cuda(), c.cuda(), lens.cuda())
    with torch.no_grad():
        m.proj.bias.add_(1.0)                # a parameter update since the forward
    with pytest.raises(RuntimeError, match="activations are gone"):
        mu3.sum().backward()


def test_no_grad_forward_is_the_inference_path(enc_sd):
    B, T = 3, 37
    tok, c, lens = text_inputs(B, T, [37, 25, 9], 21)
    m = _module(enc_sd, "f16")
    with torch.no_grad():
        a = m(tok.cuda(), c.cuda(), lens.cuda())
    x, mu_x, mask = m(tok.cuda(), c.cuda(), lens.cuda())      # training forward: same kernels up to the fused epilogues
    assert torch.equal(mask, a[2])
    assert _rel(x.detach().cpu().numpy(), a[0].cpu().numpy()) <= 1e-3
    assert _rel(mu_x.detach().cpu().numpy(), a[1].cpu().numpy()) <= 1e-3


def _ddp_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_text_encoder_ddp", os.path.join(ROOT, "tools", "train_text_encoder_ddp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_py_chain_matches_the_oracle_encoder_in_the_same_chain(enc_sd, sd):
    """models/model.py:143-177 as train.py runs it with install(text_encoder=True): native encoder -> monotonic alignment search
    -> mu_y -> prior loss + the NATIVE decoder's compute_loss -> backward, two training engines in one process.  The same chain
    with the fp32 oracle encoder in place of the native one: the same alignment, and the encoder's gradients and d c (which adds
    the decoder's and the encoder's parts) agree to the training bars."""
    from stabletts_amd.flow_matching import CFMDecoder
    tool = _ddp_tool()
    B, Tx = 3, 40
    tok, lens, c, y, y_mask = tool.make_batch(B, Tx, 93)
    lens = torch.tensor([40, 33, 21]); tok[1, 33:] = 0; tok[2, 21:] = 0      # ragged text, the mel cut where its last token ends
    ends = np.cumsum([1 + (i * 7 + 3) % 3 for i in range(Tx)])                 # (make_batch's durations)
    for b_, L_ in enumerate(lens.tolist()):
        y_mask[b_, :, int(ends[L_ - 1]):] = 0
    dec = CFMDecoder(128, 128, 256, 128, 1024, 4, 6, 3, 0.1, 256, operand_dtype="f16")
    dec.estimator.load_state_dict(sd)
    dec = dec.cuda().eval()
    g = torch.Generator().manual_seed(7)
    t_rand, z = torch.rand(B, 1, 1, generator=g).cuda(), torch.randn(*y.shape, generator=g).cuda()
    yc, ymc = y.cuda(), y_mask.cuda()
    m = _module(enc_sd, "f16")
    cn = c.cuda().clone().requires_grad_(True)
    _, mu_x, x_mask = m(tok.cuda(), cn, lens.cuda())
    ln, attn_n = tool.chain_loss(x_mask, mu_x, yc, ymc, cn, dec, t_rand, z)
    ln.backward()
    gn = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
    dec.zero_grad(set_to_none=True)
    pr = {k: v.clone().requires_grad_(True) for k, v in enc_sd.items()}
    co = c.clone().requires_grad_(True)
    _, mu_o, xm_o = oracle.text_encoder_forward(pr, tok, co, lens)
    lo, attn_o = tool.chain_loss(xm_o.cuda(), mu_o.cuda(), yc, ymc, co.cuda(), dec, t_rand, z)
    lo.backward()
    assert torch.equal(attn_n, attn_o), "the alignment search chose another path"
    _check("f16", (float(ln.detach()), cn.grad.cpu(), gn), (float(lo.detach()), co.grad, {n: p.grad for n, p in pr.items()}), "train.py chain")


def test_ddp_two_ranks_match_single_process(tmp_path):
    """DistributedDataParallel around the text encoder and the decoder together (tools/train_text_encoder_ddp.py), 2 processes
    sharing the GPU over gloo, against one process on the whole batch: per-step loss and the parameters after the steps (as
    tests/test_gpu_training.py's decoder-only DDP test).  The encoder's gradients are views of its flat buffer: they go through
    DDP's reducer like any other .grad."""
    out2, out1 = tmp_path / "ddp.pt", tmp_path / "one.pt"
    port = 29500 + (os.getpid() % 150)
    env = dict(os.environ, BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
    tool = os.path.join(ROOT, "tools", "train_text_encoder_ddp.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), tool, "--out", str(out2), "--backend", "gloo"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r1 = subprocess.run([sys.executable, tool, "--out", str(out1)], env=dict(os.environ), capture_output=True, text=True,
                        timeout=600, cwd=ROOT)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-4000:]
    a, b = torch.load(out2), torch.load(out1)
    assert a["world"] == 2 and b["world"] == 1 and len(a["losses"]) == len(b["losses"]) == 3
    print(f"[ddp] losses 2 ranks {a['losses']}, 1 process {b['losses']}")
    for la, lb in zip(a["losses"], b["losses"]):
        assert abs(la - lb) <= 2e-4 * abs(lb), (a["losses"], b["losses"])
    assert a["losses"][-1] < a["losses"][0]
    for k in a["params"]:
        assert _rel(a["params"][k].numpy(), b["params"][k].numpy()) <= 2e-3, k
