#!/usr/bin/env python
"""Are two builds of the library bitwise identical on the 16-bit decoder and text-encoder paths?
usage: python tools/grad_bitwise_ab.py [--a-captures-more] libA.so libB.so [case ...]      ("default": the library of this tree)
(developer tool: one fresh process per library and environment, one after the other, each under its own time limit; stops at the
first that fails.  The same seeds in both; compared with torch.equal on the bit patterns.)

Cases (all by default); each saves the loss, every output, every parameter gradient and every input gradient it has:
  dec_b8       decoder training step, B = 8 x T = 1000 ragged, dropout on: the phased conv tile (SiLU in the GEMM epilogues)
  dec_b3       decoder training, B = 3 x T = 300, lengths 300 / 211 / 64, dropout on, two consecutive steps (buffers reused): the
               small grid (stand-alone SiLU kernels).  Run again under each of ENV_VARIANTS, set for both libraries alike
  dec_gin128   decoder training with gin_channels = 128, B = 2 x T = 52, lengths 52 / 37: the per-block adaLN linears
  dec_parts    the B = 3 step through the engine: st_train_backward, then st_train_backward_part 0, 1, 2 into a caller's flat
               buffer; the two must agree with each other as well
  te_train     text-encoder training, gin = 192, B = 3 x T = 77 ragged, dropout on, with the loss on x and mu_x, on mu_x only
               and on x only (proj's gradient is zero-filled); B = 1 x T = 1
  te_infer     text-encoder inference, f16 and bf16, B = 2 x T = 44 ragged and B = 64 x T = 300 (the big-grid tiles)
  te_capture   text-encoder inference at B = 2 x T = 44 under debug capture: every captured tensor.  A name that only one library
               captures fails the run; with --a-captures-more (libB is the parent) libA may capture more names, never fewer
  dec_forward  one st_estimator_forward with a per-item t, B = 2 x T = 44

The launches of a library, for a kernel trace (names and call counts of two libraries must be equal): one text-encoder inference
call, one decoder training step at B = 3 x T = 300 and one text-encoder training step, in one process:
  STABLETTS_HIP_LIB=lib.so rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/grad_bitwise_ab.py --run /tmp/trace.pt trace
"""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 300
CASES = ["dec_b8", "dec_b3", "dec_gin128", "dec_parts", "te_train", "te_infer", "te_capture", "dec_forward"]
ENV_VARIANTS = ["ST_FUSE_SILU=0", "ST_FUSE_TRAIN_LN=0", "ST_TRAIN_VLO=0", "ST_TRAIN_SIDE=0"]      # each re-runs dec_b3
B3 = (3, 300, [300, 211, 64])
CAPTURE_NAMES = ["h0", "v"] + [f"b{i}.{n}" for i in range(3) for n in ("x1", "h1", "q", "k", "vt", "attn", "x2", "h2", "u", "x3")]


def _decoder(gin=256):
    import oracle
    from oracle.weights import DecoderConfig
    from stabletts_amd.flow_matching import CFMDecoder
    dec = CFMDecoder(128, 128, 256, 128, 1024, 4, 6, 3, 0.1, gin)
    dec.estimator.load_state_dict(oracle.make_state_dict(1234, DecoderConfig(gin_channels=gin)))
    return dec.cuda()


def _dec_inputs(B, T, lengths, gin=256, ragged=False):
    from oracle.inputs import make_inputs
    inp = make_inputs(B, T, seed=5, lengths=lengths, gin=gin, ragged=ragged)
    x1 = make_inputs(B, T, seed=6, gin=gin)["z"]
    g0 = torch.Generator().manual_seed(3)
    t_rand = torch.rand(B, 1, 1, generator=g0)
    z = torch.randn(B, 128, T, generator=g0)
    return inp, x1, t_rand, z


def _dec_steps(pre, dec, B, T, lengths, gin=256, ragged=False, steps=1):
    """compute_loss's chain with the estimator's input as a leaf: loss, the estimator output, d x, d mu, d c, every parameter gradient."""
    from stabletts_amd.autograd import cfm_loss, cfm_loss_prep
    inp, x1, t_rand, z = _dec_inputs(B, T, lengths, gin, ragged)
    dec.train(True)
    torch.manual_seed(77)      # (the dropout seed of every forward is drawn from torch's CPU generator)
    got = {}
    for step in range(steps):
        dec.zero_grad(set_to_none=True)
        mask = inp["mask"].cuda()
        t, y, u = cfm_loss_prep(x1.cuda(), z.cuda(), t_rand.cuda(), dec.sigma_min)
        x, mu, c = (v.clone().requires_grad_(True) for v in (y, inp["mu"].cuda(), inp["c"].cuda()))
        pred = dec.estimator(t, x, mask, mu, c)
        loss = cfm_loss(pred, u, mask)
        loss.backward()
        p = f"{pre}/step{step}"
        got.update({f"{p}/loss": loss.detach().reshape(1).cpu(), f"{p}/out": pred.detach().cpu(), f"{p}/d_x": x.grad.cpu(),
                    f"{p}/d_mu": mu.grad.cpu(), f"{p}/d_c": c.grad.cpu()})
        got.update({f"{p}/grad/{n}": q.grad.cpu() for n, q in dec.estimator.named_parameters()})
    return got


def _dec_parts(pre, dec):
    """One forward + st_train_backward, the same forward again + the three parts into a caller's buffer."""
    B, T, lengths = B3
    inp, x1, _, z = _dec_inputs(B, T, lengths)
    eng = dec.estimator.engine()
    s = torch.cuda.current_stream().cuda_stream
    f32 = dict(device="cuda", dtype=torch.float32)
    t = torch.tensor([0.2, 0.5, 0.9], **f32)
    x, mu, mask, c, g = z.cuda(), inp["mu"].cuda(), inp["mask"].cuda(), inp["c"].cuda(), x1.cuda().contiguous()
    got = {}
    for mode in ("one_call", "parts"):
        out, gx, gmu, gc = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x), torch.empty_like(c)
        flat = torch.zeros(eng.grad_layout()[None], **f32)
        eng.train_forward(t, x, mu, mask, c, out, 0.1, 12345, s)
        if mode == "one_call":
            eng.train_backward(eng.train_serial(), g, gx, gmu, gc, s)
            eng.param_grads_flat(flat, s)
        else:
            eng.train_backward_part(eng.train_serial(), 0, B, T, g, flat, None, None, None, s)
            eng.train_backward_part(eng.train_serial(), 1, B, T, None, None, None, None, None, s)
            eng.train_backward_part(eng.train_serial(), 2, B, T, None, None, gx, gmu, gc, s)
        torch.cuda.synchronize()
        got.update({f"{pre}/{mode}/out": out.cpu(), f"{pre}/{mode}/d_x": gx.cpu(), f"{pre}/{mode}/d_mu": gmu.cpu(),
                    f"{pre}/{mode}/d_c": gc.cpu(), f"{pre}/{mode}/grad_flat": flat.cpu()})
    same = all(_same(got[f"{pre}/one_call/{k}"], got[f"{pre}/parts/{k}"]) for k in ("out", "d_x", "d_mu", "d_c", "grad_flat"))
    got[f"{pre}/parts_equal_one_call"] = torch.tensor([1.0 if same else 0.0])
    return got


def _text_encoder(dt, gin, train):
    import oracle
    from oracle.weights import TextEncoderConfig
    from stabletts_amd.text_encoder import TextEncoder
    m = TextEncoder(401, 128, 256, 1024, 4, 3, 3, 0.1, gin, operand_dtype=dt)
    m.load_state_dict(oracle.make_text_encoder_state_dict(77, TextEncoderConfig(gin_channels=gin)))
    return m.cuda().train(train)


def _te_train(pre):
    import numpy as np
    from oracle.make_golden_text_encoder import text_inputs
    m = _text_encoder("f16", 192, True)
    got = {}
    for B, T, lengths, losses in ((3, 77, [77, 50, 13], ("x_mu", "mu", "x")), (1, 1, [1], ("x_mu",))):
        tok, c, lens = text_inputs(B, T, lengths, 40 + B, gin=192)
        rng = np.random.Generator(np.random.PCG64(1000 + B))
        w_mu = torch.from_numpy(rng.standard_normal((B, 128, T)).astype(np.float32)).cuda()
        w_x = torch.from_numpy((rng.standard_normal((B, 256, T)) * 0.1).astype(np.float32)).cuda()
        torch.manual_seed(78)
        for which in losses:
            m.zero_grad(set_to_none=True)
            cc = c.cuda().clone().requires_grad_(True)
            x, mu_x, mask = m(tok.cuda(), cc, lens.cuda())
            loss = ((mu_x * w_mu).sum() if "mu" in which else 0) + ((x * w_x).sum() if "x" in which.split("_") else 0)
            loss.backward()
            p = f"{pre}/B{B}_T{T}/{which}"
            got.update({f"{p}/loss": loss.detach().reshape(1).cpu(), f"{p}/x": x.detach().cpu(), f"{p}/mu_x": mu_x.detach().cpu(),
                        f"{p}/mask": mask.cpu(), f"{p}/d_c": cc.grad.cpu()})
            got.update({f"{p}/grad/{n}": q.grad.cpu() for n, q in m.named_parameters() if q.grad is not None})
    return got


def _te_infer(pre, capture=False):
    import numpy as np
    from oracle.make_golden_text_encoder import text_inputs
    got = {}
    rng = np.random.Generator(np.random.PCG64(9))
    big = [int(v) for v in rng.integers(180, 301, size=64)]
    big[5] = 300
    shapes = [(2, 44, [44, 29])] if capture else [(2, 44, [44, 29]), (64, 300, big)]
    for dt in (("f16",) if capture else ("f16", "bf16")):
        m = _text_encoder(dt, 256, False)
        if capture:
            m.engine().debug_capture(True)
        for B, T, lengths in shapes:
            tok, c, lens = text_inputs(B, T, lengths, 40 + B)
            with torch.no_grad():
                x, mu_x, mask = m(tok.cuda(), c.cuda(), lens.cuda())
            p = f"{pre}/{dt}/B{B}_T{T}"
            got.update({f"{p}/x": x.cpu(), f"{p}/mu_x": mu_x.cpu(), f"{p}/mask": mask.cpu()})
            if capture:
                from stabletts_amd._lib import NativeError
                for name in CAPTURE_NAMES:
                    try:
                        got[f"{p}/capture/{name}"] = torch.from_numpy(m.engine().debug_fetch(name))
                    except NativeError:      # this library does not capture that name
                        pass
    return got


def _dec_forward(pre, dec):
    from oracle.inputs import make_inputs
    inp = make_inputs(2, 44, seed=5, lengths=[44, 29])
    dec.eval()
    with torch.no_grad():
        out = dec.estimator(torch.tensor([0.3, 0.7]), inp["z"].cuda(), inp["mask"].cuda(), inp["mu"].cuda(), inp["c"].cuda())
    return {f"{pre}/out": out.cpu()}


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))      # bit patterns: NaN == NaN


def _trace_workload():
    """What the kernel trace of the docstring covers; nothing is compared."""
    from oracle.make_golden_text_encoder import text_inputs
    tok, c, lens = text_inputs(2, 44, [44, 29], 42)
    with torch.no_grad():
        _text_encoder("f16", 256, False)(tok.cuda(), c.cuda(), lens.cuda())
    _dec_steps("trace", _decoder(), *B3)
    m = _text_encoder("f16", 192, True)
    tok, c, lens = text_inputs(3, 77, [77, 50, 13], 43, gin=192)
    x, mu_x, _ = m(tok.cuda(), c.cuda().requires_grad_(True), lens.cuda())
    (x.sum() + mu_x.sum()).backward()
    torch.cuda.synchronize()
    return {}


def _run(cases):
    if cases == ["trace"]:
        return _trace_workload()
    got = {}
    dec = _decoder() if any(c in cases for c in ("dec_b8", "dec_b3", "dec_parts", "dec_forward")) else None
    if "dec_b8" in cases:
        got.update(_dec_steps("dec_b8", dec, 8, 1000, None, ragged=True))
    if "dec_b3" in cases:
        got.update(_dec_steps("dec_b3", dec, *B3, steps=2))
    if "dec_parts" in cases:
        got.update(_dec_parts("dec_parts", dec))
    if "dec_forward" in cases:
        got.update(_dec_forward("dec_forward", dec))
    if "dec_gin128" in cases:
        got.update(_dec_steps("dec_gin128", _decoder(128), 2, 52, [52, 37], gin=128))
    if "te_train" in cases:
        got.update(_te_train("te_train"))
    if "te_infer" in cases:
        got.update(_te_infer("te_infer"))
    if "te_capture" in cases:
        got.update(_te_infer("te_capture", capture=True))
    torch.cuda.synchronize()
    return got


if len(sys.argv) == 4 and sys.argv[1] == "--run":
    sys.path.insert(0, ROOT)
    torch.save(_run(sys.argv[3].split(",")), sys.argv[2])
    sys.exit(0)
a_captures_more = "--a-captures-more" in sys.argv
sys.argv = [a for a in sys.argv if a != "--a-captures-more"]
if len(sys.argv) < 3:
    sys.exit(__doc__)
cases = sys.argv[3:] or CASES
unknown = [c for c in cases if c not in CASES]
if unknown:
    sys.exit(f"unknown case(s) {unknown}: one of {CASES}")
groups = [("", cases)] + ([(v, ["dec_b3"]) for v in ENV_VARIANTS] if "dec_b3" in cases else [])
failed = False
for var, group_cases in groups:
    outs = []
    for i, lib in enumerate(sys.argv[1:3]):
        path = f"/tmp/grad_ab_{os.getpid()}_{i}.pt"
        env = dict(os.environ)
        if lib != "default":
            env["STABLETTS_HIP_LIB"] = os.path.abspath(lib)
        if var:
            env[var.split("=")[0]] = var.split("=")[1]
        rc = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--run", path,
                             ",".join(group_cases)], env=env).returncode
        if rc != 0:
            sys.exit(f"the run with {lib} [{var or 'default environment'}] failed (exit {rc}): stopping")
        outs.append(torch.load(path))
        os.remove(path)
    a, b = outs
    missing = sorted(n for n in b if n not in a)
    extra = sorted(n for n in a if n not in b)
    allowed = [n for n in extra if a_captures_more and "/capture/" in n]
    missing += [n for n in extra if n not in allowed]
    diff = [n for n in b if n in a and not _same(a[n], b[n])]
    unequal_parts = [n for r in (a, b) for n in r if n.endswith("parts_equal_one_call") and float(r[n]) != 1.0]
    for case in group_cases:
        names = [n for n in b if n.startswith(case + "/") and n in a]
        print(f"[{var or 'default environment'}] {case}: {len(names)} tensors compared, {sum(n in diff for n in names)} differ", flush=True)
    if allowed:
        print(f"  captured by [{sys.argv[1]}] only (--a-captures-more): {allowed}")
    if missing or diff or unequal_parts:
        failed = True
        print(f"  DIFFERENT: {diff[:8]}  missing from one run: {missing[:8]}  backward in parts != one call: {unequal_parts}")
print(f"[{sys.argv[1]}] vs [{sys.argv[2]}]: " + ("DIFFERENCES FOUND" if failed else "bit-identical on every case"))
sys.exit(1 if failed else 0)
