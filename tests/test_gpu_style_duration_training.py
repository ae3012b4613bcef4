"""Native training of the MelStyleEncoder and the DurationPredictor (st_style_encoder_train_* / st_duration_predictor_train_*
behind stabletts_amd._fp32_module's autograd Functions, opted in with native_training) on a real MI355X: gradients against the
REAL reference modules (tests/golden/style_dp_grads.npz, tools/make_golden_style_dp_grads.py), the p = 0 forward against the
inference forward, counter-based dropout against the torch restatement run on the same masks, determinism, the error paths,
AdamW steps and train.py's loss chain with every module native.  Run with ``-m gpu``.

Both modules train in fp32 (the fp32-input MFMA and VALU row kernels), so the gate is near fp32 rounding:
max |native - ref| / max |ref| <= 1e-4 per tensor.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import style_dp_restatement as R  # noqa: E402
import synth_weights as sw  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.grad]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-4
WORST = {}


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "style_dp_grads.npz"))


def _style(dropout=0.25):
    from stabletts_amd.reference_encoder_train import MelStyleEncoder
    m = MelStyleEncoder(sw.N_MELS, style_vector_dim=sw.GIN, style_kernel_size=5, dropout=dropout)
    m.load_state_dict(sw.style_encoder_state_dict(), strict=True)
    return m.cuda()


def _dp():
    from stabletts_amd.duration_predictor_train import DurationPredictor
    m = DurationPredictor(sw.DP_HIDDEN, sw.DP_FILTER, sw.DP_KERNEL, 0.5, sw.GIN)
    m.load_state_dict(sw.duration_predictor_state_dict(), strict=True)
    return m.cuda()


def _style_in(B, T, lengths, seed):
    y, m = sw.style_inputs(B, T, lengths, seed)
    return torch.from_numpy(y).cuda(), (torch.from_numpy(m).cuda() if m is not None else None)


def _dp_in(B, T, lengths, seed):
    return tuple(torch.from_numpy(a).cuda() for a in sw.dp_inputs(B, T, lengths, seed))


def _check_against_gold(gold, case, mod, loss):
    ref_loss = float(gold[f"{case}/loss"][()])
    assert abs(float(loss) - ref_loss) <= 1e-5 * max(abs(ref_loss), 1.0), (case, float(loss), ref_loss)
    names = gold[f"{case}/names"].tolist()
    absmax = gold[f"{case}/absmax"]
    grads = {n: p.grad.detach().reshape(-1).cpu().numpy() for n, p in mod.named_parameters()}
    assert sorted(grads) == names
    worst = {}
    for i, n in enumerate(names):
        g = grads[n]
        if f"{case}/full/{n}" in gold.files:
            ref = gold[f"{case}/full/{n}"]
            nat = g
        else:
            ref = gold[f"{case}/sample/{n}"]
            seed = (R.STYLE_GRAD_CASES.get(case) or R.DP_GRAD_CASES[case])[3]
            nat = g[R.sample_index(g.size, seed + i)]
        worst[n] = float(np.abs(nat.astype(np.float64) - ref).max() / max(float(absmax[i]), 1e-30))
        nrm = float(np.linalg.norm(g.astype(np.float64)))
        assert abs(nrm - float(gold[f"{case}/norms"][i])) <= 1e-4 * max(float(gold[f"{case}/norms"][i]), 1e-30), (case, n)
    WORST[case] = max(worst.values())
    print(f"{case}: worst max|d| / max|ref| = {WORST[case]:.2e} ({max(worst, key=worst.get)})")
    bad = {k: v for k, v in worst.items() if v > GATE}
    assert not bad, (case, bad)


# ---- 1. gradients of the real reference modules
@pytest.mark.parametrize("case", list(R.STYLE_GRAD_CASES))
def test_style_encoder_gradients_match_reference(gold, case):
    B, T, lengths, seed = R.STYLE_GRAD_CASES[case]
    m = _style().eval()
    y, mask = _style_in(B, T, lengths, seed)
    c = m(y, mask)
    loss = (c * R.loss_weights(tuple(c.shape), seed).cuda()).sum()
    loss.backward()
    _check_against_gold(gold, case, m, loss.item())


@pytest.mark.parametrize("case", list(R.DP_GRAD_CASES))
def test_duration_predictor_gradients_match_reference(gold, case):
    B, T, lengths, seed = R.DP_GRAD_CASES[case]
    m = _dp().eval()
    x, mask, g = _dp_in(B, T, lengths, seed)
    logw = m(x, mask, g)
    loss = (logw * R.loss_weights(tuple(logw.shape), seed).cuda()).sum()
    loss.backward()
    _check_against_gold(gold, case, m, loss.item())


# ---- 2. p = 0: the training forward is the inference forward, bit for bit
def test_training_forward_at_p0_equals_inference_forward():
    """The DurationPredictor's p = 0 training forward is bitwise the inference forward.  The style encoder's is not yet: its c
    differs in the last bits (measured <= 9e-8 absolute on c of magnitude ~1); gated at 1e-6 of max |c| here."""
    s, d = _style().eval(), _dp().eval()
    for B, T, lengths, seed in R.STYLE_GRAD_CASES.values():
        y, mask = _style_in(B, T, lengths, seed)
        c_tr = s(y, mask)
        assert c_tr.requires_grad
        with torch.no_grad():
            c_inf = s(y, mask)
        rel = _rel(c_tr.detach().cpu(), c_inf.cpu())
        print(f"style p0 training vs inference: {rel:.2e}, bitwise {torch.equal(c_tr.detach(), c_inf)}")
        assert rel <= 1e-6
    for B, T, lengths, seed in R.DP_GRAD_CASES.values():
        x, mask, g = _dp_in(B, T, lengths, seed)
        l_tr = d(x, mask, g)
        with torch.no_grad():
            l_inf = d(x, mask, g)
        assert torch.equal(l_tr.detach(), l_inf)


# ---- 3. dropout: the native masks rebuilt in numpy, the restatement run on them
def _native_seed(torch_seed):
    torch.manual_seed(torch_seed)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def test_style_encoder_dropout_matches_restatement_with_same_masks():
    B, T, lengths, seed = R.STYLE_GRAD_CASES["se_b3_t37"]
    m = _style().train()
    y, mask = _style_in(B, T, lengths, seed)
    w = R.loss_weights((B, sw.GIN), seed).cuda()
    losses = []
    for ts in (5, 5, 6):
        m.zero_grad()
        torch.manual_seed(ts)
        loss = (m(y, mask) * w).sum()
        loss.backward()
        losses.append(loss.item())
    assert losses[0] == losses[1] and losses[0] != losses[2]
    m.zero_grad()
    torch.manual_seed(5)
    (m(y, mask) * w).sum().backward()
    drops = R.style_drops(_native_seed(5), 0.25, B, sw.STYLE_HIDDEN, T)
    for k in ("spec0", "glu1"):
        kept = float((drops[k] > 0).float().mean())
        assert abs(kept - 0.75) < 0.01, (k, kept)
    sd = {k: v.clone().requires_grad_(True) for k, v in sw.style_encoder_state_dict().items()}
    c = R.style_forward(sd, y.cpu(), mask.cpu(), drop=drops)
    ref_loss = (c * w.cpu()).sum()
    ref_loss.backward()
    assert abs(losses[0] - ref_loss.item()) <= 1e-5 * max(abs(ref_loss.item()), 1.0)
    worst = {n: _rel(p.grad.cpu(), sd[n].grad) for n, p in m.named_parameters()}
    print("style dropout worst", max(worst.values()))
    assert max(worst.values()) <= GATE, worst


def test_duration_predictor_dropout_matches_restatement_with_same_masks():
    B, T, lengths, seed = R.DP_GRAD_CASES["dp_b3_t37"]
    m = _dp().train()
    x, mask, g = _dp_in(B, T, lengths, seed)
    w = R.loss_weights((B, 1, T), seed).cuda()
    losses = []
    for ts in (7, 7, 8):
        m.zero_grad()
        torch.manual_seed(ts)
        loss = (m(x, mask, g) * w).sum()
        loss.backward()
        losses.append(loss.item())
    assert losses[0] == losses[1] and losses[0] != losses[2]
    m.zero_grad()
    torch.manual_seed(7)
    (m(x, mask, g) * w).sum().backward()
    drops = R.dp_drops(_native_seed(7), 0.5, B, sw.DP_FILTER, T)
    kept = float((drops["norm1"] > 0).float().mean())
    assert abs(kept - 0.5) < 0.01, kept
    sd = {k: v.clone().requires_grad_(True) for k, v in sw.duration_predictor_state_dict().items()}
    ref_loss = (R.dp_forward(sd, x.cpu(), mask.cpu(), g.cpu(), drop=drops) * w.cpu()).sum()
    ref_loss.backward()
    assert abs(losses[0] - ref_loss.item()) <= 1e-5 * max(abs(ref_loss.item()), 1.0)
    worst = {n: _rel(p.grad.cpu(), sd[n].grad) for n, p in m.named_parameters()}
    print("dp dropout worst", max(worst.values()))
    assert max(worst.values()) <= GATE, worst


# ---- 4. bitwise repeatable gradients (no atomics), at train.py's largest shapes too
@pytest.mark.parametrize("B,T", [(3, 37), (64, 333)])
def test_style_encoder_gradients_are_bitwise_repeatable(B, T):
    m = _style().eval()
    lengths = [T - (i * 7) % (T // 2) for i in range(B)]
    y, mask = _style_in(B, T, lengths, 99)
    w = torch.randn(B, sw.GIN, generator=torch.Generator().manual_seed(1)).cuda()
    grads = []
    for _ in range(2):
        m.zero_grad()
        (m(y, mask) * w).sum().backward()
        grads.append([p.grad.clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    assert all(torch.isfinite(a).all() for a in grads[0])


@pytest.mark.parametrize("B,T", [(3, 37), (64, 200)])
def test_duration_predictor_gradients_are_bitwise_repeatable(B, T):
    m = _dp().eval()
    lengths = [T - (i * 7) % (T // 2) for i in range(B)]
    x, mask, g = _dp_in(B, T, lengths, 98)
    w = torch.randn(B, 1, T, generator=torch.Generator().manual_seed(2)).cuda()
    grads = []
    for _ in range(2):
        m.zero_grad()
        (m(x, mask, g) * w).sum().backward()
        grads.append([p.grad.clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


# ---- 5. error paths and the opt-in
def test_stale_backward_no_grad_path_and_default_class():
    m = _style().eval()
    y, mask = _style_in(3, 37, [37, 20, 5], 13)
    c1 = m(y, mask)
    c2 = m(y, mask)
    with pytest.raises(RuntimeError, match="activations are gone"):
        c1.sum().backward()
    c2.sum().backward()
    c3 = m(y, mask)
    with torch.no_grad():
        m.fc.bias.add_(0.0)                       # an in-place parameter update bumps the version
    with pytest.raises(RuntimeError, match="activations are gone"):
        c3.sum().backward()
    d = _dp().eval()
    x, xm, g = _dp_in(3, 37, [37, 25, 9], 21)
    l1 = d(x, xm, g)
    d(x, xm, g)
    with pytest.raises(RuntimeError, match="activations are gone"):
        l1.sum().backward()
    # no_grad on a trainable instance = the inference path of the default class
    from stabletts_amd.duration_predictor import DurationPredictor
    from stabletts_amd.reference_encoder import MelStyleEncoder
    base = MelStyleEncoder(sw.N_MELS, style_vector_dim=sw.GIN, style_kernel_size=5, dropout=0.25)
    base.load_state_dict(sw.style_encoder_state_dict())
    base = base.cuda().train()
    with torch.no_grad():
        assert torch.equal(m.train()(y, mask), base(y, mask))
    assert MelStyleEncoder.native_training is False and DurationPredictor.native_training is False
    with pytest.raises(NotImplementedError):
        base(y, mask)


def test_train_entry_points_reject_other_kinds_and_nulls():
    s, d = _style(), _dp()
    lib = s.engine().lib
    se, de = s.engine().handle, d.engine().handle
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    assert lib.st_style_encoder_train_forward(de, p, None, p, 1, 1, 0.0, 0, None) == -3
    assert lib.st_duration_predictor_train_forward(se, p, p, p, p, 1, 1, 0.0, 0, None) == -3
    assert lib.st_style_encoder_train_backward(de, 1, 1, 1, p, p, None) == -3
    assert lib.st_duration_predictor_train_backward(se, 1, 1, 1, p, p, None) == -3
    assert lib.st_style_encoder_train_forward(se, None, None, p, 1, 1, 0.0, 0, None) == -1
    assert lib.st_duration_predictor_train_forward(de, p, None, p, p, 1, 1, 0.0, 0, None) == -1
    assert lib.st_style_encoder_train_backward(se, 1, 1, 1, None, p, None) == -1
    assert lib.st_style_encoder_train_backward(se, 1, 1, 1, p, p, None) == -3       # no forward held


# ---- 6. AdamW steps against the restatement (eval mode: no dropout)
def _adamw_run(mod_params, steps, loss_fn):
    opt = torch.optim.AdamW(mod_params, lr=1e-3, weight_decay=0.01)
    for _ in range(steps):
        opt.zero_grad()
        loss_fn().backward()
        opt.step()


def test_adamw_steps_follow_restatement():
    B, T, lengths, seed = R.STYLE_GRAD_CASES["se_b3_t37"]
    m = _style().eval()
    y, mask = _style_in(B, T, lengths, seed)
    w = R.loss_weights((B, sw.GIN), seed).cuda()
    eng = m.engine()
    p0 = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    sizes = []
    for _ in range(5):
        opt.zero_grad()
        (m(y, mask) * w).sum().backward()
        opt.step()
        sizes.append(m.engine().device_bytes())
    assert m.engine() is eng and len(set(sizes)) == 1, sizes
    sd = {k: v.clone().requires_grad_(True) for k, v in sw.style_encoder_state_dict().items()}
    _adamw_run(list(sd.values()), 5, lambda: (R.style_forward(sd, y.cpu(), mask.cpu()) * w.cpu()).sum())
    H = sw.STYLE_HIDDEN
    for n, p in m.named_parameters():
        a = (p.detach().cpu() - p0[n].cpu()).double().reshape(-1)
        b = (sd[n].detach() - p0[n].cpu()).double().reshape(-1)
        if n == "slf_attn.in_proj_bias":
            # the k bias adds one constant to every score of a softmax row: its gradient is 0 up to rounding noise, which
            # AdamW normalises into +-lr steps of random sign (in torch as natively); compare the q and v parts
            keep = torch.cat([torch.arange(0, H), torch.arange(2 * H, 3 * H)])
            a, b = a[keep], b[keep]
        cos = float(a @ b / max(float(a.norm() * b.norm()), 1e-30))
        assert cos >= 0.999, (n, cos)
    d = _dp().eval()
    x, xm, g = _dp_in(3, 37, [37, 25, 9], 21)
    wl = R.loss_weights((3, 1, 37), 21).cuda()
    q0 = {n: p.detach().clone() for n, p in d.named_parameters()}
    _adamw_run(d.parameters(), 5, lambda: (d(x, xm, g) * wl).sum())
    sd = {k: v.clone().requires_grad_(True) for k, v in sw.duration_predictor_state_dict().items()}
    _adamw_run(list(sd.values()), 5, lambda: (R.dp_forward(sd, x.cpu(), xm.cpu(), g.cpu()) * wl.cpu()).sum())
    for n, p in d.named_parameters():
        a = (p.detach().cpu() - q0[n].cpu()).double().reshape(-1)
        b = (sd[n].detach() - q0[n].cpu()).double().reshape(-1)
        cos = float(a @ b / max(float(a.norm() * b.norm()), 1e-30))
        assert cos >= 0.999, (n, cos)


# ---- 7. train.py's chain (models/model.py:114-178) with every module native
def test_train_chain_with_every_module_native():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle
    from stabletts_amd.duration_predictor import duration_loss
    from stabletts_amd.flow_matching import CFMDecoder
    from stabletts_amd.text_encoder import TextEncoder
    from train_text_encoder_ddp import chain_loss
    torch.manual_seed(0)
    B, Tx, Ty, Tz = 3, 30, 90, 60
    enc = TextEncoder(401, 128, 256, 1024, 4, 3, 3, 0.1, 256).cuda().eval()
    enc.load_state_dict(oracle.make_text_encoder_state_dict(2468))
    dec = CFMDecoder(128, 128, 256, 128, 1024, 4, 6, 3, 0.1, 256).cuda().eval()
    dec.estimator.load_state_dict(oracle.make_state_dict(1234))
    style, dp = _style().eval(), _dp().eval()
    fake_speaker = torch.zeros(1, 256, device="cuda", requires_grad=True)
    gen = torch.Generator().manual_seed(3)
    tok = torch.randint(1, 401, (B, Tx), generator=gen).cuda()
    x_len = torch.tensor([30, 22, 14]).cuda()
    y = torch.randn(B, 128, Ty, generator=gen).cuda()
    y_len = torch.tensor([90, 70, 45]).cuda()
    y_mask = (torch.arange(Ty, device="cuda")[None] < y_len[:, None]).float().unsqueeze(1)
    z = y[:, :, :Tz].contiguous()
    z_mask = (torch.arange(Tz, device="cuda")[None] < torch.tensor([60, 50, 30], device="cuda")[:, None]).float().unsqueeze(1)
    cfg_mask = torch.tensor([[True], [False], [True]], device="cuda")
    t_rand = torch.rand(B, generator=gen).cuda()
    noise = torch.randn(B, 128, Ty, generator=gen).cuda()

    def run(style_fn, dp_fn):
        c = style_fn(z, z_mask) * cfg_mask + ~cfg_mask * fake_speaker.repeat(B, 1)
        x, mu_x, x_mask = enc(tok, c, x_len)
        logw = dp_fn(x, x_mask, c)
        rest, attn = chain_loss(x_mask, mu_x, y, y_mask, c, dec, t_rand, noise)
        logw_ = torch.log(1e-8 + attn.sum(2)) * x_mask
        return duration_loss(logw, logw_, x_len) + rest, attn

    loss, attn = run(style, dp)
    loss.backward()
    g_nat = {("s", n): p.grad.detach().cpu() for n, p in style.named_parameters()}
    g_nat.update({("d", n): p.grad.detach().cpu() for n, p in dp.named_parameters()})
    # The restatement chain, twice.  Free: its own c / logw flow on (the text encoder and the decoder have 16-bit operands, so
    # the 1e-6 difference of c moves their backward by more than the fp32 gate: reported, gated loosely).  Pinned: the forward
    # values are the native chain's (value of the native output, gradient through the restatement), which isolates the two
    # modules' backward: gated at the fp32 gate.
    with torch.no_grad():
        c_nat = style(z, z_mask)
        c_used = c_nat * cfg_mask + ~cfg_mask * fake_speaker.repeat(B, 1)
        x_nat, _, xm_nat = enc(tok, c_used, x_len)
        logw_nat = dp(x_nat, xm_nat, c_used)
    for pinned in (False, True):
        ssd = {k: v.cuda().requires_grad_(True) for k, v in sw.style_encoder_state_dict().items()}
        dsd = {k: v.cuda().requires_grad_(True) for k, v in sw.duration_predictor_state_dict().items()}

        def sf(a, b):
            c = R.style_forward(ssd, a, b)
            return c + (c_nat - c).detach() if pinned else c

        def df(a, b, c):
            lw = R.dp_forward(dsd, a, b, c)
            return lw + (logw_nat - lw).detach() if pinned else lw

        loss_r, attn_r = run(sf, df)
        loss_r.backward()
        assert torch.equal(attn, attn_r)
        worst = {k: _rel(v, (ssd if k[0] == "s" else dsd)[k[1]].grad.cpu()) for k, v in g_nat.items()}
        print("chain", "pinned" if pinned else "free", "worst", max(worst.values()), "loss", loss.item(), loss_r.item())
        gate = GATE if pinned else 2e-3
        assert max(worst.values()) <= gate, {k: v for k, v in worst.items() if v > gate}
    assert math.isfinite(loss.item())


# ---- 8. DDP: 2 gloo ranks on one GPU against one process on the whole batch
def test_ddp_two_ranks_match_single_process(tmp_path):
    import subprocess
    out2, out1 = tmp_path / "ddp.pt", tmp_path / "one.pt"
    port = 29650 + (os.getpid() % 150)
    tool = os.path.join(ROOT, "tools", "train_style_dp_ddp.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), tool, "--out", str(out2), "--backend", "gloo"]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r1 = subprocess.run([sys.executable, tool, "--out", str(out1)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-4000:]
    a, b = torch.load(out2), torch.load(out1)
    assert a["world"] == 2 and b["world"] == 1 and len(a["losses"]) == len(b["losses"]) == 3
    print(f"[ddp] losses 2 ranks {a['losses']}, 1 process {b['losses']}")
    for la, lb in zip(a["losses"], b["losses"]):
        assert abs(la - lb) <= 1e-4 * max(abs(lb), 1.0), (a["losses"], b["losses"])
    assert a["losses"][-1] < a["losses"][0]
    for k in a["params"]:
        assert _rel(a["params"][k].numpy(), b["params"][k].numpy()) <= 1e-4, k
