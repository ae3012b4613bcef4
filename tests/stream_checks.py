"""Every native entry point on a non-blocking side stream, behind work that is still pending (tests/test_gpu_stream_order.py,
tools/stream_order.py).

The rest of the suite never leaves the legacy default stream, which orders itself with every blocking stream, uploads its inputs
with synchronous copies and leaves the right answer in the workspaces for a second run.  A launch, memset or table upload issued
on stream 0 instead of the stream argument, a child stream forked before the caller's pending work or joined too late, a host read
that does not wait for the caller's stream, a workspace that a kernel refilled too early: none of them can fail there.

``behind_pending_work`` runs one entry point three times on the same device buffers:

1. expected: inputs A, default stream, twice (the second run establishes that the entry repeats bit for bit);
2. poison: other inputs B of the same shapes on a fresh non-blocking stream S (first-use allocations and one-time
   synchronisations happen here, and every workspace, slot and kept activation now holds another problem's values); then the
   float inputs are overwritten with NaN.  Masks and integer inputs (tokens, lengths, durations) keep B's valid values, so
   that a kernel that ran early cannot index outside a buffer;
3. checked: on S, in this order, a delay kernel of about 100 ms, an event ``gate``, device-to-device copies of A into the
   buffers, the entry point.  ``pending = not gate.query()`` right after the call returned on the host says that the whole
   call was enqueued while S was still blocked: anything that did not wait for S read NaN, B or stale values.  The outputs
   must equal step 1 bit for bit (``torch.equal`` on an int32 view).

The delay is a harness parameter, calibrated once per process with two events, not a gate on the code.

``GPU_MAX_HW_QUEUES`` is left as the environment sets it.  With few hardware queues a wrongly addressed launch can land in the
queue that is sleeping and run in order by accident: the suite cannot see a wrong-stream launch that happens to share a hardware
queue with the sleeping stream.  That can only hide a bug; it cannot produce a false failure.

``CASES`` maps a case id to a builder of its ``Problem``; each case builds its own module or engine.  The builders reuse those of
the families' own tests at their smallest shapes.  ``HOST_SYNCHRONISING`` lists the cases whose call is documented to block the
host ("Streams"), each with the line that blocks; every other case asserts ``pending``.
"""
import dataclasses
import functools
import os
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEV = "cuda:0"
TARGET_MS = 100.0
DELAY_RANGE_MS = (50.0, 500.0)

# case id -> the line that blocks the host.  Only entries that INTEGRATION.md's "Streams" paragraph names as synchronising.
HOST_SYNCHRONISING = {
    "decoder_dopri5": "stabletts_amd/csrc/engine_solve.cpp:108 hipStreamSynchronize(s): the adaptive controller reads the step's error norm",
    "vocos_repack": "stabletts_amd/_native_module.py:125 torch.cuda.synchronize(dev): an inference vocoder re-loads its parameters after an update",
    "gan_discriminator_loss": "stabletts_amd/gan_loss.py:268 means.tolist(): the per-discriminator losses are returned as Python floats",
}


# ---- the delay -------------------------------------------------------------------------------------------------------------------
class _Delay:
    """About TARGET_MS of work on the current stream: torch.cuda._sleep, or a chain of fp32 matmuls where that is unusable."""

    def __init__(self):
        self.kind, self.count, self.x = "sleep", 0, None
        try:
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
            n = 10_000_000
            unit = self._time(lambda: torch.cuda._sleep(n)) / n
        except (AttributeError, RuntimeError):
            self.kind = "matmul"
            self.x = torch.randn(4096, 4096, device=DEV)
            self.y = torch.empty_like(self.x)
            self._chain(2)
            torch.cuda.synchronize()
            unit = self._time(lambda: self._chain(8)) / 8
        self.count = max(1, int(TARGET_MS / unit))
        self.ms = self._time(self.enqueue)

    def _chain(self, k):
        for _ in range(k):
            torch.mm(self.x, self.x, out=self.y)

    @staticmethod
    def _time(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def enqueue(self):
        if self.kind == "sleep":
            torch.cuda._sleep(self.count)
        else:
            self._chain(self.count)


@functools.lru_cache(maxsize=None)
def delay():
    d = _Delay()
    assert DELAY_RANGE_MS[0] <= d.ms <= DELAY_RANGE_MS[1], f"the delay kernel measures {d.ms:.1f} ms ({d.kind} x {d.count}): mis-calibrated"
    return d


# ---- the protocol ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Problem:
    """fn(bufs) makes the native call on the current stream and returns its output tensors (any nesting of lists).  a / b: the
    two problems' inputs by name (same shapes and dtypes).  bufs: the device buffers, where the case must own them (the
    optimizer's parameters); else they are allocated here.  keep: float inputs that keep B's values instead of NaN (masks).
    expected_fn / poison_fn: what steps 1 and 2 run where that is not fn (the re-pack cases).  outside(outs): run after the
    stream context is left, with the default stream current; its result replaces fn's."""
    fn: callable
    a: dict
    b: dict
    bufs: dict = None
    keep: tuple = ()
    expected_fn: callable = None
    poison_fn: callable = None
    outside: callable = None


@dataclasses.dataclass
class Result:
    pending: bool
    bitwise: bool
    repeats: bool
    host_ms: float
    delay_ms: float
    mismatched: list
    outputs: list
    expected: list
    stream: object = None       # (kept alive with the result, so that the next fresh stream is another one)


def flat(outs):
    if torch.is_tensor(outs):
        return [outs]
    if isinstance(outs, dict):
        outs = list(outs.values())
    if isinstance(outs, (list, tuple)):
        return [t for o in outs for t in flat(o)]
    return []       # (Python floats, None)


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _fill(bufs, src):
    with torch.no_grad():
        for k, t in bufs.items():
            t.copy_(src[k])


def _poison(bufs, keep):
    with torch.no_grad():
        for k, t in bufs.items():
            if t.dtype.is_floating_point and k not in keep and "mask" not in k:
                t.fill_(float("nan"))


def behind_pending_work(p):
    d = delay()
    a = {k: v.to(DEV) for k, v in p.a.items()}
    b = {k: v.to(DEV) for k, v in p.b.items()}
    assert set(a) == set(b) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
    bufs = p.bufs if p.bufs is not None else {k: torch.empty_like(v) for k, v in a.items()}
    outside = p.outside or (lambda outs: outs)
    expected_fn = p.expected_fn or p.fn
    # 1. expected, on the default stream, twice
    runs = []
    for _ in range(2):
        _fill(bufs, a)
        outs = flat(outside(expected_fn(bufs)))
        torch.cuda.synchronize()
        runs.append([o.detach().clone() for o in outs])
    expected = runs[0]
    repeats = len(runs[0]) == len(runs[1]) and all(same_bits(x, y) for x, y in zip(*runs))
    # 2. another problem on the side stream: first-use allocations, other values in every workspace; then NaN inputs
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(s):
        _fill(bufs, b)
        outs = (p.poison_fn or p.fn)(bufs)
    outs = outside(outs)
    torch.cuda.synchronize()
    del outs
    _poison(bufs, p.keep)
    torch.cuda.synchronize()
    # 3. the call behind pending work
    gate = torch.cuda.Event()
    with torch.cuda.stream(s):
        d.enqueue()
        gate.record(s)
        _fill(bufs, a)
        t0 = time.perf_counter()
        outs = p.fn(bufs)
        host_ms = (time.perf_counter() - t0) * 1e3
    pending = not gate.query()
    outs = flat(outside(outs))
    s.synchronize()
    torch.cuda.synchronize()
    mismatched = [i for i, (x, y) in enumerate(zip(outs, expected)) if not same_bits(x.detach(), y)]
    bitwise = len(outs) == len(expected) and len(outs) > 0 and not mismatched
    return Result(pending, bitwise, repeats, host_ms, d.ms, mismatched, [o.detach() for o in outs], expected, s)


def check(case):
    """Runs a case and asserts what the issue asks: bitwise equality, and ``pending`` unless the case is allowlisted."""
    r = behind_pending_work(CASES[case]())
    print(row(case, r))
    assert r.repeats, f"{case}: two runs on the default stream differ"
    assert r.bitwise, f"{case}: outputs {r.mismatched} of {len(r.expected)} differ from the default-stream run"
    if case not in HOST_SYNCHRONISING:
        assert r.pending, f"{case}: the call blocked the host until the stream's pending work had finished ({r.host_ms:.1f} ms)"
    return r


def row(case, r):
    yn = lambda v: "yes" if v else "no"         # noqa: E731
    line = f"{case:34s} delay {r.delay_ms:6.1f} ms  host {r.host_ms:8.2f} ms  pending {yn(r.pending):3s}  repeats {yn(r.repeats):3s}  bitwise {yn(r.bitwise):3s}"
    if case in HOST_SYNCHRONISING:
        line += "  [" + HOST_SYNCHRONISING[case] + "]"
    return line


# ---- helpers of the cases --------------------------------------------------------------------------------------------------------
def _t(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))


def _inference(call):
    def fn(bufs):
        with torch.no_grad():
            return call(bufs)
    return fn


def _training(mods, call, leaves=(), seed=None):
    """fn: zero the gradients, one grad-enabled forward, the backward of the sum of squares of every differentiable output;
    -> those outputs, the gradients of the `leaves` inputs and every parameter gradient."""
    mods = mods if isinstance(mods, (list, tuple)) else [mods]

    def forward(bufs):
        for m in mods:
            m.zero_grad(set_to_none=True)
        if seed is not None:
            torch.manual_seed(seed)         # (train mode: the counter-based dropout is seeded from torch's CPU generator)
        lv = {k: bufs[k].detach().requires_grad_(True) for k in leaves}
        outs = [o for o in flat(call({**bufs, **lv})) if o.requires_grad]
        loss = outs[0].square().sum()
        for o in outs[1:]:
            loss = loss + o.square().sum()
        return lv, outs, loss

    def collect(lv, outs):
        return ([o.detach() for o in outs] + [lv[k].grad for k in leaves]
                + [q.grad for m in mods for q in m.parameters() if q.grad is not None])

    def fn(bufs):
        with torch.enable_grad():
            lv, outs, loss = forward(bufs)
            loss.backward()
        return collect(lv, outs)

    fn.forward, fn.collect = forward, collect
    return fn


def _env(name, value, fn):
    def wrapped(bufs):
        old = os.environ.get(name)
        os.environ[name] = value
        try:
            return fn(bufs)
        finally:
            if old is None:
                del os.environ[name]
            else:
                os.environ[name] = old
    return wrapped


def _two_weights(mod):
    ws = [q for _, q in mod.named_parameters() if q.dim() >= 2]
    return ws[0], ws[-1]


def _scale_two(mod):
    with torch.no_grad():
        for q in _two_weights(mod):
            q.mul_(1.01)


# ---- decoder ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decoder_weights():
    import oracle
    return oracle.make_state_dict(1234), oracle.make_cfg_params(4321)


def _decoder(train=False):
    from test_gpu_training import _decoder as build
    return build(_decoder_weights()[0], "f16", train=train)


def _decoder_inputs(B, T, seed, lengths):
    from oracle.inputs import make_inputs
    inp = make_inputs(B, T, seed=seed, lengths=lengths)
    return {k: inp[k] for k in ("mu", "mask", "c", "z")}


def _solve_call(dec, n, solver, cfg):
    fs, fc = _decoder_weights()[1]
    kw = dict(fake_speaker=fs.to(DEV), fake_content=fc.to(DEV), cfg_strength=cfg) if cfg is not None else None
    return lambda t: dec(t["mu"], t["mask"], n, 1.0, t["c"], solver, kw, z=t["z"])


def _solve(n, solver, cfg, B=2, T=70, la=(70, 51), lb=(64, 70), split=None):
    def build():
        fn = _inference(_solve_call(_decoder(), n, solver, cfg))
        if split is not None:
            fn = _env("ST_SPLIT", split, fn)
        return Problem(fn, _decoder_inputs(B, T, 21, list(la)), _decoder_inputs(B, T, 22, list(lb)))
    return build


def _estimator():
    dec = _decoder()
    a, b = _decoder_inputs(2, 70, 23, [70, 51]), _decoder_inputs(2, 70, 24, [64, 70])
    a["t"], b["t"] = torch.tensor([0.4]), torch.tensor([0.7])       # (a device tensor: a host scalar is a pageable upload)
    return Problem(_inference(lambda t: dec.estimator(t["t"], t["z"], t["mask"], t["mu"], t["c"])), a, b)


def _decoder_repack():
    """Two parameters scaled in place on S behind the delay, then a solve: the re-pack kernels (st_repack) run on S behind the
    update.  Expected from a second module that was built with the scaled weights."""
    dec, scaled = _decoder(), _decoder()
    _scale_two(scaled.estimator)
    torch.cuda.synchronize()
    solve, solve_scaled = (_inference(_solve_call(d, 4, "euler", 3.0)) for d in (dec, scaled))

    def fn(bufs):
        _scale_two(dec.estimator)
        return solve(bufs)

    return Problem(fn, _decoder_inputs(2, 70, 25, [70, 51]), _decoder_inputs(2, 70, 26, [64, 70]), expected_fn=solve_scaled, poison_fn=solve)


def _decoder_training_inputs(B, T, seed, lengths):
    from oracle.inputs import make_inputs
    inp = make_inputs(B, T, seed=seed, lengths=lengths)
    g = torch.Generator().manual_seed(seed)
    return dict(mu=inp["mu"], mask=inp["mask"], c=inp["c"], x1=make_inputs(B, T, seed=seed + 100)["z"],
                t_rand=torch.rand(B, 1, 1, generator=g), z=torch.randn(B, 128, T, generator=g))


def _decoder_training():
    dec = _decoder(train=True)
    call = lambda t: dec.compute_loss(t["x1"], t["mask"], t["mu"], t["c"], t_rand=t["t_rand"], z=t["z"])[0]        # noqa: E731
    return Problem(_training(dec, call, leaves=("mu", "c"), seed=500),
                   _decoder_training_inputs(2, 44, 31, [44, 29]), _decoder_training_inputs(2, 44, 32, [40, 44]))


# ---- text encoder, style encoder, duration predictor -----------------------------------------------------------------------------
def _text_inputs(seed, lengths):
    from oracle.make_golden_text_encoder import text_inputs
    tok, c, lens = text_inputs(2, 33, lengths, seed)
    return dict(tok=_t(tok), c=_t(c), lens=_t(lens))


def _text_encoder(train):
    def build():
        import oracle
        import text_encoder_checks as tec
        from oracle.weights import TextEncoderConfig
        m = tec.module(TextEncoderConfig(), oracle.make_text_encoder_state_dict(2468), "f16")
        call = lambda t: m(t["tok"], t["c"], t["lens"])         # noqa: E731
        fn = _training(m, call, leaves=("c",)) if train else _inference(call)
        return Problem(fn, _text_inputs(41, [33, 20]), _text_inputs(42, [27, 33]))
    return build


def _style_inputs(seed, lengths):
    import synth_weights as sw
    y, m = sw.style_inputs(3, 37, lengths, seed)
    return dict(y=_t(y), mask=_t(m))


def _dp_inputs(seed, lengths):
    import synth_weights as sw
    x, m, g = sw.dp_inputs(3, 37, lengths, seed)
    return dict(x=_t(x), mask=_t(m), g=_t(g))


def _style(train):
    def build():
        if train:
            from test_gpu_style_duration_training import _style as make
            m = make().eval()
        else:
            import synth_weights as sw
            from stabletts_amd.reference_encoder import MelStyleEncoder
            m = MelStyleEncoder(sw.N_MELS, style_vector_dim=sw.GIN, style_kernel_size=5, dropout=0.25)
            m.load_state_dict(sw.style_encoder_state_dict(), strict=True)
            m = m.cuda()
        call = lambda t: m(t["y"], t["mask"])       # noqa: E731
        return Problem(_training(m, call) if train else _inference(call), _style_inputs(13, [37, 20, 5]), _style_inputs(14, [9, 37, 30]))
    return build


def _duration(train):
    def build():
        if train:
            from test_gpu_style_duration_training import _dp as make
            m = make().eval()
        else:
            import synth_weights as sw
            from stabletts_amd.duration_predictor import DurationPredictor
            m = DurationPredictor(sw.DP_HIDDEN, sw.DP_FILTER, sw.DP_KERNEL, 0.5, sw.GIN)
            m.load_state_dict(sw.duration_predictor_state_dict(), strict=True)
            m = m.cuda()
        call = lambda t: m(t["x"], t["mask"], t["g"])       # noqa: E731
        return Problem(_training(m, call) if train else _inference(call), _dp_inputs(21, [37, 25, 9]), _dp_inputs(22, [12, 37, 31]))
    return build


# ---- Vocos, FireflyGAN -----------------------------------------------------------------------------------------------------------
def _vocos_module(train=False, M=64):
    from oracle import vocos_oracle as vo
    cfg = vo.vocos_config(input_channels=M, intermediate_dim=256, num_layers=2)
    if train:
        from stabletts_amd.vocos_train import Vocos
    else:
        from stabletts_amd.vocos import Vocos
    m = Vocos(types.SimpleNamespace(input_channels=cfg.input_channels, dim=cfg.dim, intermediate_dim=cfg.intermediate_dim, num_layers=cfg.num_layers),
              types.SimpleNamespace(n_fft=cfg.n_fft, hop_length=cfg.hop_length))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vo.make_vocos_state_dict(77, cfg).items()}, strict=True)
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _mel(seed, M=64, B=2, T=7):
    from oracle import vocos_oracle as vo
    return dict(mel=_t(vo.make_mel(B, T, seed, M=M)))


def _vocos():
    m = _vocos_module()
    return Problem(_inference(lambda t: m(t["mel"])), _mel(51), _mel(52))


def _vocos_ragged():
    """Host lengths [7, 3]; the poison run vocodes [6, 7] (more packed rows, so the checked run allocates nothing)."""
    m = _vocos_module()
    return Problem(_inference(lambda t: m.forward_ragged(t["mel"], [7, 3])), _mel(53), _mel(54),
                   poison_fn=_inference(lambda t: m.forward_ragged(t["mel"], [6, 7])))


def _vocos_training():
    m = _vocos_module(train=True)
    return Problem(_training(m, lambda t: m(t["mel"]), leaves=("mel",)), _mel(55), _mel(56))


def _vocos_backward_outside():
    """The training forward on S behind the delay; backward() is called after the stream context is left, with the default
    stream current.  The Functions take torch.cuda.current_stream() inside backward and rely on autograd restoring the
    forward's stream."""
    m = _vocos_module(train=True)
    tr = _training(m, lambda t: m(t["mel"]), leaves=("mel",))

    def fn(bufs):
        with torch.enable_grad():
            return tr.forward(bufs)

    def outside(state):
        lv, outs, loss = state
        loss.backward()
        return tr.collect(lv, outs)

    return Problem(fn, _mel(57), _mel(58), outside=outside)


def _vocos_repack():
    m, scaled = _vocos_module(), _vocos_module()
    _scale_two(scaled)
    torch.cuda.synchronize()
    run, run_scaled = (_inference(lambda t, v=v: v(t["mel"])) for v in (m, scaled))

    def fn(bufs):
        _scale_two(m)
        return run(bufs)

    return Problem(fn, _mel(59), _mel(60), expected_fn=run_scaled, poison_fn=run)


def _solve_then_vocos():
    """Two calls behind one delay, the chain synthesise runs: an Euler solve, then a Vocos forward on its output."""
    dec, voc = _decoder(), _vocos_module(M=128)
    solve = _solve_call(dec, 4, "euler", 3.0)
    return Problem(_inference(lambda t: voc(solve(t))), _decoder_inputs(2, 70, 27, [70, 51]), _decoder_inputs(2, 70, 28, [64, 70]))


def _ffgan_mel(seed):
    from tests import ffgan_restatement as fr
    return dict(mel=fr.make_mel(2, 33, 64, seed))


def _ffgan(ragged):
    def build():
        import ffgan_checks as fc
        m, _ = fc.build(fc.SMALL, "f16")
        if not ragged:
            return Problem(_inference(lambda t: m(t["mel"])), _ffgan_mel(3), _ffgan_mel(4))
        return Problem(_inference(lambda t: m.forward_ragged(t["mel"], [33, 17])), _ffgan_mel(5), _ffgan_mel(6),
                       poison_fn=_inference(lambda t: m.forward_ragged(t["mel"], [30, 33])))
    return build


# ---- log-mel, resample -----------------------------------------------------------------------------------------------------------
def _waves(seed, sizes):
    g = torch.Generator().manual_seed(seed)
    return {f"w{i}": 0.3 * torch.randn(*n, generator=g) for i, n in enumerate(sizes)}


def _log_mel(train=False):
    if train:
        from stabletts_amd.audio_train import LogMelSpectrogram
    else:
        from stabletts_amd.audio import LogMelSpectrogram
    return LogMelSpectrogram(44100, 256, 256, 64, 0.0, None, 96, 40, False, "reflect", "slaney").to(DEV)


def _mel_forward():
    m = _log_mel()
    return Problem(_inference(lambda t: m(t["w0"])), _waves(61, [(2, 2000)]), _waves(62, [(2, 2000)]))


def _mel_ragged():
    """Two ragged calls in a row: two slots of the utterance-table ring are in flight behind one delay."""
    m = _log_mel()
    sizes = [(2000,), (1500,), (777,)]
    call = lambda t: [m.forward_ragged([t["w0"], t["w1"], t["w2"]]), m.forward_ragged([t["w2"], t["w0"]])]     # noqa: E731
    return Problem(_inference(call), _waves(63, sizes), _waves(64, sizes))


def _mel_backward():
    m = _log_mel(train=True)
    return Problem(_training(m, lambda t: m(t["w0"]), leaves=("w0",)), _waves(65, [(2, 2000)]), _waves(66, [(2, 2000)]))


def _resample():
    from stabletts_amd.audio import resample
    return Problem(_inference(lambda t: resample(t["w0"], 48000, 44100)), _waves(67, [(2, 777)]), _waves(68, [(2, 777)]))


def _resample_ragged():
    from stabletts_amd.audio import resample_ragged
    sizes = [(777,), (500,), (123,)]
    return Problem(_inference(lambda t: resample_ragged([t["w0"], t["w1"], t["w2"]], 48000, 44100)), _waves(69, sizes), _waves(70, sizes))


# ---- discriminators and the GAN losses -------------------------------------------------------------------------------------------
def _mpd_module():
    from tests import mpd_restatement as R
    from stabletts_amd.discriminator import MultiPeriodDiscriminator
    m = MultiPeriodDiscriminator((2, 3))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.make_mpd_state_dict(301, (2, 3)).items()}, strict=True)
    return m.to(DEV).train()


def _mrd_module():
    from tests import mrd_restatement as R
    from stabletts_amd.discriminator import MultiResolutionDiscriminator
    sizes = (64, 32)
    m = MultiResolutionDiscriminator(sizes)
    m.load_state_dict({k: _t(v) for k, v in R.with_windows(R.make_mrd_state_dict(401, sizes), sizes).items()}, strict=True)
    return m.to(DEV).train()


def _pair(T, seed):
    from tests import mpd_restatement as R
    return dict(y=_t(R.make_audio(2, T, seed)), y_hat=_t(R.make_audio(2, T, seed + 1)))


def _discriminator(make, T, seed):
    def build():
        m = make()
        return Problem(_training(m, lambda t: m(t["y"], t["y_hat"]), leaves=("y_hat",)), _pair(T, seed), _pair(T, seed + 10))
    return build


def _gan_losses(which):
    """The fused losses on the period discriminator's maps (the two halves of one base: the node's fast path), with their
    backward through the discriminator."""
    def build():
        from stabletts_amd import gan_loss as G
        m = _mpd_module()

        def call(t):
            y_d_rs, y_d_gs, fmap_rs, fmap_gs = m(t["y"], t["y_hat"])
            if which == "discriminator":
                return G.discriminator_loss(y_d_rs, y_d_gs)[0]
            return [G.feature_loss(fmap_rs, fmap_gs), G.generator_loss(y_d_gs)[0]]

        return Problem(_training(m, call, leaves=("y_hat",)), _pair(99, 81), _pair(99, 91))
    return build


# ---- optimizer -------------------------------------------------------------------------------------------------------------------
def _adamw():
    """AdamW.step over the parity counts (one parameter and one gradient 4-byte aligned only, one empty tensor).  The parameters,
    gradients and moments are the buffers: every run restores them and the step count."""
    import test_gpu_optim as tgo
    from stabletts_amd.optim import AdamW
    counts = tgo.parity_counts()
    ps = [tgo._leaf(tgo._rand(n, 100 + i), odd=bool(po)) for i, (n, po, _) in enumerate(counts)]
    for i, (p, (n, _, go)) in enumerate(zip(ps, counts)):
        p.grad = tgo._place(tgo._rand(n, 1000 + i, scale=0.5 + i), odd=bool(go))
    opt = AdamW([dict(params=ps[:5], **tgo.GROUP_A), dict(params=ps[5:], **tgo.GROUP_B)])
    assert opt._native_device() == torch.device(DEV)
    opt.step()              # (creates the state)
    torch.cuda.synchronize()
    bufs, a, b = {}, {}, {}
    for i, p in enumerate(ps):
        st = opt.state[p]
        for j, (name, t, scale) in enumerate((("p", p.detach(), 1.0), ("g", p.grad, 0.5 + i), ("m", st["exp_avg"], 0.1), ("v", st["exp_avg_sq"], 0.01))):
            bufs[f"{name}{i}"] = t
            for dst, seed in ((a, 2000), (b, 3000)):
                r = tgo._rand(t.numel(), seed + 10 * i + j, scale=scale)
                dst[f"{name}{i}"] = r.square() if name == "v" else r

    def fn(_):
        for p in ps:
            opt.state[p]["step"].fill_(3.0)
        opt.step()
        return [[p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]] for p in ps]

    return Problem(fn, a, b, bufs=bufs)


def _clip(max_norm):
    def build():
        import test_gpu_optim as tgo
        from stabletts_amd.optim import clip_grad_norm_
        ps = tgo._grad_list(seed=1, scale=2.0)
        with_grad = [p for p in ps if p.grad is not None]
        bufs = {f"g{i}": p.grad for i, p in enumerate(with_grad)}
        a, b = ({k: tgo._rand(t.numel(), seed + i, scale=2.0) for i, (k, t) in enumerate(bufs.items())} for seed in (4000, 5000))

        def fn(_):
            with torch.no_grad():
                norm = clip_grad_norm_(ps, max_norm)
            return [norm] + [p.grad for p in with_grad]

        return Problem(fn, a, b, bufs=bufs)
    return build


# ---- alignment -------------------------------------------------------------------------------------------------------------------
def _flip(d):
    """Another valid problem of the same shapes: the batch in reverse order, the floats halved."""
    out = {}
    for k, v in d.items():
        w = v.flip(0) if v.dim() > 1 or k.endswith("lengths") else v
        out[k] = w * 0.5 if w.dtype.is_floating_point and "mask" not in k else w.clone()
    return out


def _maximum_path():
    from stabletts_amd.monotonic_align import maximum_path
    gold = np.load(os.path.join(HERE, "golden", "mas_outputs.npz"))
    a = dict(neg_cent=_t(gold["ragged/neg_cent"]), mask=_t(gold["ragged/mask"]))
    return Problem(_inference(lambda t: maximum_path(t["neg_cent"], t["mask"])), a, _flip(a))


def _align_and_losses():
    from tests import align_loss_restatement as ar
    from stabletts_amd.alignment import align_and_losses
    g = ar.case_of(dict(np.load(ar.GOLDEN)), "ragged")
    names = ("mu_x", "x_mask", "logw", "x_lengths", "y", "y_mask", "durations", "keep", "fake_content")
    a = {k: _t(g[k]) for k in names}

    def call(t):
        out = align_and_losses(t["mu_x"], t["x_mask"], t["logw"], t["x_lengths"], t["y"], t["y_mask"], t["durations"], keep=t["keep"],
                               fake_content=t["fake_content"])
        return [out["mu_y_masked"], out["prior_loss"], out["dur_loss"], out["mu_y"]]

    return Problem(_training([], call, leaves=("mu_x", "logw", "fake_content")), a, _flip(a), keep=("keep",))


# ---- the positive control --------------------------------------------------------------------------------------------------------
def wrong_stream_op():
    """Plain torch, no native code: x * 2 issued on the default stream whatever stream is current.  A benign data race on
    allocated memory: the protocol must report a mismatch with `pending` true."""
    def fn(bufs):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return bufs["x"] * 2
    g = torch.Generator().manual_seed(1)
    return Problem(fn, dict(x=torch.randn(1 << 16, generator=g)), dict(x=torch.randn(1 << 16, generator=g)))


def positive_control(max_streams=8):
    """The protocol on wrong_stream_op, on up to `max_streams` fresh side streams that all stay alive: the runtime maps streams
    onto a few hardware queues, and a side stream that shares the default stream's queue runs the planted op in order, which
    hides it (the module docstring's blind spot).  -> the results; the last one is the first that shows the mismatch, if any
    did.  Every attempt must have returned with the stream still blocked."""
    results = []
    for _ in range(max_streams):
        results.append(behind_pending_work(wrong_stream_op()))
        if not results[-1].bitwise:
            break
    return results


CASES = {
    "decoder_estimator": _estimator,
    "decoder_euler_cfg": _solve(4, "euler", 3.0),
    "decoder_rk4": _solve(2, "rk4", None),
    "decoder_euler_cfg_split2": _solve(4, "euler", 3.0, split="2"),
    "decoder_dopri5": _solve(10, "dopri5", None, B=1, T=12, la=(12,), lb=(9,)),
    "decoder_repack": _decoder_repack,
    "decoder_training": _decoder_training,
    "text_encoder": _text_encoder(False),
    "text_encoder_training": _text_encoder(True),
    "style_encoder": _style(False),
    "style_encoder_training": _style(True),
    "duration_predictor": _duration(False),
    "duration_predictor_training": _duration(True),
    "vocos": _vocos,
    "vocos_ragged": _vocos_ragged,
    "vocos_training": _vocos_training,
    "vocos_repack": _vocos_repack,
    "vocos_backward_outside": _vocos_backward_outside,
    "solve_then_vocos": _solve_then_vocos,
    "ffgan": _ffgan(False),
    "ffgan_ragged": _ffgan(True),
    "mel": _mel_forward,
    "mel_ragged_twice": _mel_ragged,
    "mel_backward": _mel_backward,
    "resample": _resample,
    "resample_ragged": _resample_ragged,
    "mpd_training": _discriminator(_mpd_module, 99, 71),
    "mrd_training": _discriminator(_mrd_module, 97, 75),
    "gan_feature_generator_loss": _gan_losses("feature_generator"),
    "gan_discriminator_loss": _gan_losses("discriminator"),
    "adamw_step": _adamw,
    "clip_grad_norm_above": _clip(1.0),
    "clip_grad_norm_below": _clip(1000.0),
    "maximum_path": _maximum_path,
    "align_and_losses": _align_and_losses,
}
TRAINING = {c for c in CASES if c.endswith("_training") or c in ("vocos_backward_outside", "mel_backward", "gan_feature_generator_loss",
                                                                "gan_discriminator_loss", "align_and_losses")}
