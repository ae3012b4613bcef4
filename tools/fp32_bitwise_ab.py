#!/usr/bin/env python
"""Are two builds of the library bitwise identical on the fp32 handle kinds and the two vocoders?  usage: python tools/fp32_bitwise_ab.py libA.so libB.so
(developer tool: one fresh process per library, one after the other, each under its own time limit; stops at the first that fails.)

Compared with torch.equal, at the shapes of the GPU tests (tile edges, every tap count, Cin / Cout off the 16 / 64 multiples,
split-K weight gradients):
  style encoder / duration predictor   the inference output, and the training forward's output and every parameter (and input)
                                       gradient in eval mode and with dropout on, for synth_weights.STYLE_ALL_CASES / DP_ALL_CASES
  Vocos training                       waveform, parameter gradients and d mel at (B, T) = (2, 1), (2, 3), (2, 61), (1, 20) and
                                       (2, 9) with input_channels 128, on the small_linear configuration and weights
  period discriminator                 feature maps, d x and parameter gradients at every shape of tests/test_gpu_mpd.py: SHAPES
  resolution discriminator, mel extractor, Vocos inference, FireflyGAN inference
                                       one case each through the C ABI, at the configurations and shapes of
                                       tests/test_gpu_handle_lifecycle.py; the resolution discriminator also through one training
                                       forward and backward (feature maps, d x, every parameter gradient).  The configurations,
                                       weights and forwards are imported from that test module (as the period discriminator's
                                       shapes are from its own), so an edit there changes what is compared here.  These are the
                                       smallest shapes each kind accepts: B = 1, T = 8 frames (97 samples for the discriminator, 64
                                       for the mel extractor), and the mel extractor and the two vocoders compare ONE output
                                       tensor each -- a check that moved host code still launches the same work, not a sweep
                                       of tile paths (tests/test_gpu_vocoder.py, test_gpu_mel.py and test_gpu_ffgan.py are that).
                                       Each vocoder also runs its ragged entry point once on the same handle: one chunk, B = 3,
                                       T = 40, lengths (40, 17, 1)
"""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 600
RAGGED_B, RAGGED_T, RAGGED_LENGTHS = 3, 40, (40, 17, 1)
VOCOS_SHAPES = [(2, 1, {}), (2, 3, {}), (2, 61, {}), (1, 20, {}), (2, 9, dict(input_channels=128))]


def _backward(out, mod, loss, inputs, pre):
    """{name: tensor} of one forward + backward: the outputs, every parameter gradient, the gradient of every input that has one."""
    outs = list(out) if isinstance(out, (list, tuple)) else [out]
    got = {f"{pre}/out{i}": o.detach().cpu() for i, o in enumerate(outs)}
    mod.zero_grad(set_to_none=True)
    loss.backward()
    got.update({f"{pre}/grad/{n}": p.grad.cpu() for n, p in mod.named_parameters() if p.grad is not None})
    got.update({f"{pre}/d_in{i}": x.grad.cpu() for i, x in enumerate(inputs) if x.grad is not None})
    return got


def _style_dp():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import style_dp_restatement as R
    import synth_weights as sw
    from stabletts_amd import duration_predictor, duration_predictor_train, reference_encoder, reference_encoder_train
    got = {}
    for case, (cfg, B, T, _, seed) in sw.STYLE_ALL_CASES.items():
        y, m = (torch.from_numpy(a).cuda() for a in sw.style_config_inputs(case))
        for train in (False, True):
            cls = (reference_encoder_train if train else reference_encoder).MelStyleEncoder
            mod = cls(cfg[0], style_hidden=cfg[1], style_vector_dim=cfg[2], style_kernel_size=cfg[3], style_head=cfg[4], dropout=0.25)
            mod.load_state_dict(sw.style_config_state_dict(cfg), strict=True)
            mod = mod.cuda()
            if not train:
                with torch.no_grad():
                    got[f"style/{case}/inference"] = mod(y, m).cpu()
                continue
            w = R.loss_weights((B, cfg[2]), seed).cuda()
            for mode in ("eval", "dropout"):
                mod.train(mode == "dropout")
                torch.manual_seed(seed)
                yg = y.clone().requires_grad_(True)
                c = mod(yg, m)
                got.update(_backward(c, mod, (c * w).sum(), [yg], f"style/{case}/{mode}"))
    for case, (cfg, B, T, _, seed, _) in sw.DP_ALL_CASES.items():
        x, m, g = (torch.from_numpy(a).cuda() for a in sw.dp_config_inputs(case))
        for train in (False, True):
            mod = (duration_predictor_train if train else duration_predictor).DurationPredictor(cfg[0], cfg[1], cfg[2], 0.5, cfg[3])
            mod.load_state_dict(sw.dp_config_state_dict(case), strict=True)
            mod = mod.cuda()
            if not train:
                with torch.no_grad():
                    got[f"dp/{case}/inference"] = mod(x, m, g).cpu()
                continue
            w = R.loss_weights((B, 1, T), seed).cuda()
            for mode in ("eval", "dropout"):
                mod.train(mode == "dropout")
                torch.manual_seed(seed)
                xg, gg = x.clone().requires_grad_(True), g.clone().requires_grad_(True)
                logw = mod(xg, m, gg)
                got.update(_backward(logw, mod, (logw * w).sum(), [xg, gg], f"dp/{case}/{mode}"))
    return got


def _vocos():
    import types
    from oracle import vocos_oracle as vo
    from stabletts_amd.vocos_train import Vocos
    from tests import vocos_vjp_restatement as R
    fields, _, _, wseed, mseed, _ = R.CASES["small_linear"]
    got = {}
    for B, T, over in VOCOS_SHAPES:
        cfg = vo.vocos_config(**{**fields, **over})
        mod = Vocos(types.SimpleNamespace(input_channels=cfg.input_channels, dim=cfg.dim, intermediate_dim=cfg.intermediate_dim,
                                          num_layers=cfg.num_layers), types.SimpleNamespace(n_fft=cfg.n_fft, hop_length=cfg.hop_length))
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in vo.make_vocos_state_dict(wseed, cfg).items()}, strict=True)
        mod = mod.to("cuda:0").train()
        mel = torch.from_numpy(vo.make_mel(B, T, mseed, M=cfg.input_channels)).cuda().requires_grad_(True)
        audio = mod(mel)
        W = torch.from_numpy(R.loss_weights((B, T * cfg.hop_length), wseed)).cuda()
        got.update(_backward(audio, mod, (audio * W).sum(), [mel], f"vocos/B{B}_T{T}_M{cfg.input_channels}"))
    return got


def _mpd():
    from stabletts_amd.discriminator import DiscriminatorP
    from tests import mpd_restatement as R
    from tests.test_gpu_mpd import SHAPES
    got = {}
    for p, B, T in SHAPES:
        wseed, aseed = 400 + p, 500 + T
        d = DiscriminatorP(p, lrelu_slope=0.1)
        d.load_state_dict({k: torch.from_numpy(v) for k, v in R.make_dp_state_dict(wseed).items()}, strict=True)
        d = d.to("cuda:0").train()
        x = torch.from_numpy(R.make_audio(B, T, aseed)).cuda().requires_grad_(True)
        _, fmap = d(x)
        got.update(_backward(fmap, d, R.linear_loss(fmap, wseed), [x], f"mpd/p{p}_B{B}_T{T}"))
    return got


def _other_kinds():
    from tests import test_gpu_handle_lifecycle as L
    got = {}
    for name in ("resolution_disc", "mel_extractor", "vocoder", "ffgan"):
        kind = L.KINDS[name]
        eng = kind.create()
        eng.load_state_dict(L._tensors(kind.weights(eng)))
        got.update({f"{name}/out{i}": t.cpu() for i, t in enumerate(kind.forward(eng))})
        if name == "resolution_disc":
            shapes = kind.shapes(eng, L.B)
            x, fmaps = L._rand((L.B, 1, kind.T), 10), [torch.empty(s, device="cuda") for s in shapes]
            eng.resolution_disc_forward(x, fmaps, True, None)
            d_x, flat = torch.empty_like(x), torch.zeros(eng.grad_layout()[None], device="cuda")
            eng.resolution_disc_train_backward(L.B, kind.T, [L._rand(s, 20 + i) for i, s in enumerate(shapes)], d_x, flat, None)
            got.update({f"{name}/train/out{i}": t.cpu() for i, t in enumerate(fmaps)})
            got.update({f"{name}/train/d_x": d_x.cpu(), f"{name}/train/grad_flat": flat.cpu()})
        if name in ("vocoder", "ffgan"):      # the ragged entry point, one chunk: utterances at full, odd and unit length
            M, hop = (L.VOCOS["input_channels"], L.VOCOS["hop_length"]) if name == "vocoder" else \
                (L.FFGAN["backbone"]["input_channels"], L.FFGAN["head"]["hop_length"])
            audio = torch.zeros(RAGGED_B, RAGGED_T * hop, device="cuda")
            ragged = eng.vocos_forward_ragged if name == "vocoder" else eng.ffgan_forward_ragged
            ragged(L._rand((RAGGED_B, M, RAGGED_T), 30), RAGGED_LENGTHS, audio, None)
            got[f"{name}/ragged/out0"] = audio.cpu()
        torch.cuda.synchronize()
        eng.close()
    return got


if len(sys.argv) == 3 and sys.argv[1] == "--run":
    sys.path.insert(0, ROOT)
    out = {}
    for part in (_style_dp, _vocos, _mpd, _other_kinds):
        out.update(part())
    torch.cuda.synchronize()
    torch.save(out, sys.argv[2])
    sys.exit(0)
if len(sys.argv) != 3:
    sys.exit(__doc__)
outs = []
for i, lib in enumerate(sys.argv[1:3]):
    path = f"/tmp/fp32_ab_{os.getpid()}_{i}.pt"
    env = dict(os.environ)
    if lib != "default":
        env["STABLETTS_HIP_LIB"] = os.path.abspath(lib)
    rc = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--run", path], env=env).returncode
    if rc != 0:
        sys.exit(f"the run with {lib} failed (exit {rc}): stopping")
    outs.append(torch.load(path))
    os.remove(path)
a, b = outs
assert sorted(a) == sorted(b), "the two runs saved different tensor names"
diff = [n for n in a if not torch.equal(a[n].view(torch.int32), b[n].view(torch.int32))]      # bit patterns: NaN == NaN
for group in ("style", "dp", "vocos", "mpd", "resolution_disc", "mel_extractor", "vocoder", "ffgan"):
    names = [n for n in a if n.startswith(group + "/")]
    print(f"{group}: {len(names)} tensors compared, {sum(n in diff for n in names)} differ")
print(f"[{sys.argv[1]}] vs [{sys.argv[2]}]: {len(a)} tensors, differing: {len(diff)} {diff[:8]}")
sys.exit(1 if diff else 0)
