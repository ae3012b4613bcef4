"""One walk through the life of a handle of every kind, at the C ABI: create, st_device_bytes, load, st_finalize, forward, st_finalize
again, the same forward (bitwise), st_device_bytes again (re-finalising leaks nothing into the count), st_repack (ST_OK or the kind's
refusal), and for the kinds that hold the activations of one training forward a matching backward and one with another B, destroy.
Each kind at the smallest configuration its own test file uses, B = 1; a handle of another kind comes and goes in between.
Every call is one the API defines a result for."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ffgan_restatement as ffr
from tests import mel_checks
from tests import mpd_restatement as mpd
from tests import mrd_restatement as mrd
from tests import synth_weights as sw

pytestmark = pytest.mark.gpu

B, T = 1, 8
DIT = (8, 256, 128, 4, 2, 3, 256)       # noise, hidden, filter, heads, layers, kernel, gin
N_VOCAB = 10
VOCOS = dict(input_channels=64, dim=512, intermediate_dim=256, num_layers=1, n_fft=2048, hop_length=512)
STYLE = dict(n_mel_channels=8, style_hidden=64, style_vector_dim=8, style_kernel_size=1, style_head=1)
DP = dict(in_channels=8, filter_channels=128, kernel_size=1, gin_channels=8)
MEL = dict(n_fft=32, win_length=32, hop_length=8, pad=12, n_mels=4, center=0, pad_mode=0)
MEL_L = 64
PD = dict(period=3, lrelu_slope=0.1)
PD_T = 97
RD_W, RD_T = 32, 97
RD = dict(window_length=RD_W, lrelu_slope=mrd.SLOPE, **{f"band_{k}{c}": r[j] for c, r in enumerate(mrd.band_ranges(RD_W)) for j, k in enumerate(("lo", "hi"))})
FFGAN = ffr.small_config()

IN_PLACE = "st_repack: style-encoder / duration-predictor handles read their parameters in place"
VOCODER = "st_repack: vocoder handles re-pack through st_finalize"
MEL_BANK = "st_repack: mel-extractor handles re-read their filter bank through st_finalize"


def _seeded(eng, seed):
    """Seeded weights for the kinds without a helper: U(-b, b), b = fan_in ** -0.5, by the handle's own parameter table."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for name, shape in eng.param_info():
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else int(shape[0])
        sd[name] = torch.from_numpy(rng.uniform(-1.0, 1.0, size=shape).astype(np.float32) * max(fan_in, 1) ** -0.5)
    return sd


def _rand(shape, seed):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32)).cuda()


def _tensors(sd):
    return {k: torch.as_tensor(v) for k, v in sd.items()}


class Kind:
    """create() -> Engine; weights(eng) -> state dict; forward(eng) -> output tensors; repack: ST_OK or the refusal text;
    train(eng, lib): (matching backward's code, code of the backward with B + 1, its message) or None."""
    repack = None
    train = None


class Decoder(Kind):
    def create(self):
        from stabletts_amd import _lib
        return _lib.Engine(*DIT)

    def weights(self, eng):
        return _seeded(eng, 11)

    def forward(self, eng):
        M, G = DIT[0], DIT[6]
        out = torch.empty(B, M, T, device="cuda")
        eng.estimator_forward(torch.full((1,), 0.25, device="cuda"), _rand((B, M, T), 1), _rand((B, M, T), 2), torch.ones(B, 1, T, device="cuda"),
                              _rand((B, G), 3), out, None)
        return [out]


class TextEncoder(Kind):
    def create(self):
        from stabletts_amd import _lib
        return _lib.Engine(*DIT, text_encoder_vocab=N_VOCAB)

    def weights(self, eng):
        return _seeded(eng, 12)

    def forward(self, eng):
        M, C, G = DIT[0], DIT[1], DIT[6]
        tokens = (torch.arange(B * T, device="cuda") % N_VOCAB).reshape(B, T)
        outs = [torch.empty(B, C, T, device="cuda"), torch.empty(B, M, T, device="cuda"), torch.empty(B, 1, T, device="cuda")]
        eng.text_encoder_forward(tokens, torch.full((B,), T, dtype=torch.int64, device="cuda"), _rand((B, G), 4), *outs, None)
        return outs


class Vocoder(Kind):
    repack = VOCODER

    def create(self):
        from stabletts_amd import _lib
        return _lib.Engine(*DIT, vocoder=VOCOS)

    def weights(self, eng):
        return _seeded(eng, 13)

    def forward(self, eng):
        audio = torch.empty(B, T * VOCOS["hop_length"], device="cuda")
        eng.vocos_forward(_rand((B, VOCOS["input_channels"], T), 5), audio, None)
        return [audio]

    def train(self, eng, lib):
        mel, audio = _rand((B, VOCOS["input_channels"], T), 5), torch.empty(B, T * VOCOS["hop_length"], device="cuda")
        eng.vocos_train_forward(mel, audio, None)
        flat = torch.zeros(eng.grad_layout()[None], device="cuda")
        d_audio = torch.ones(B + 1, T * VOCOS["hop_length"], device="cuda")
        call = lambda b: lib.st_vocos_train_backward(eng.handle, d_audio.data_ptr(), None, flat.data_ptr(), b, T, None)      # noqa: E731
        return call(B), call(B + 1), f"st_vocos_train_backward: the engine holds the activations of a forward with B={B}, T={T}, not B={B + 1}, T={T}"


class StyleEncoder(Kind):
    repack = IN_PLACE

    def create(self):
        from stabletts_amd import _lib
        return _lib.Engine(*DIT, style_encoder=STYLE)

    def weights(self, eng):
        return sw.style_encoder_state_dict(n_mels=STYLE["n_mel_channels"], hidden=STYLE["style_hidden"], gin=STYLE["style_vector_dim"],
                                           kernel=STYLE["style_kernel_size"])

    def forward(self, eng):
        c = torch.empty(B, STYLE["style_vector_dim"], device="cuda")
        eng.style_encoder_forward(_rand((B, STYLE["n_mel_channels"], T), 6), None, c, None)
        return [c]

    def train(self, eng, lib):
        mel, c = _rand((B, STYLE["n_mel_channels"], T), 6), torch.empty(B, STYLE["style_vector_dim"], device="cuda")
        eng.style_encoder_train_forward(mel, None, c, 0.0, 0, None)
        n = eng.train_serial()
        flat, g = torch.zeros(eng.grad_layout()[None], device="cuda"), torch.ones(B + 1, STYLE["style_vector_dim"], device="cuda")
        call = lambda b: lib.st_style_encoder_train_backward(eng.handle, n, b, T, g.data_ptr(), flat.data_ptr(), None)      # noqa: E731
        return call(B), call(B + 1), (f"st_style_encoder_train_backward: the engine holds the activations of forward #{n} (B={B}, T={T}), "
                                      f"not of #{n} (B={B + 1}, T={T})")


class DurationPredictor(Kind):
    repack = IN_PLACE

    def create(self):
        from stabletts_amd import _lib
        return _lib.Engine(*DIT, duration_predictor=DP)

    def weights(self, eng):
        return sw.duration_predictor_state_dict(hidden=DP["in_channels"], filt=DP["filter_channels"], kernel=DP["kernel_size"], gin=DP["gin_channels"])

    def _inputs(self, b):
        return _rand((b, DP["in_channels"], T), 7), torch.ones(b, 1, T, device="cuda"), _rand((b, DP["gin_channels"], 1), 8), torch.empty(b, 1, T, device="cuda")

    def forward(self, eng):
        x, m, g, logw = self._inputs(B)
        eng.duration_predictor_forward(x, m, g, logw, None)
        return [logw]

    def train(self, eng, lib):
        x, m, g, logw = self._inputs(B)
        eng.duration_predictor_train_forward(x, m, g, logw, 0.0, 0, None)
        n = eng.train_serial()
        flat, d = torch.zeros(eng.grad_layout()[None], device="cuda"), torch.ones(B + 1, 1, T, device="cuda")
        call = lambda b: lib.st_duration_predictor_train_backward(eng.handle, n, b, T, d.data_ptr(), flat.data_ptr(), None)      # noqa: E731
        return call(B), call(B + 1), (f"st_duration_predictor_train_backward: the engine holds the activations of forward #{n} (B={B}, Tx={T}), "
                                      f"not of #{n} (B={B + 1}, Tx={T})")


class MelExtractor(Kind):
    repack = MEL_BANK

    def create(self):
        from stabletts_amd import _lib
        return _lib.Engine(*DIT, mel=MEL)

    def weights(self, eng):
        return {"spectrogram.window": mel_checks.window(MEL["n_fft"]), "mel_scale.fb": mel_checks.slaney(MEL["n_fft"], MEL["n_mels"])}

    def forward(self, eng):
        out = torch.empty(B, MEL["n_mels"], eng.mel_frames(MEL_L), device="cuda")
        eng.mel_forward(torch.from_numpy(mel_checks.waves(B, MEL_L, 9)).cuda(), out, None)
        return [out]


class _Disc(Kind):
    def forward(self, eng):
        fmaps = [torch.empty(s, device="cuda") for s in self.shapes(eng, B)]
        self.fwd(eng)(_rand((B, 1, self.T), 10), fmaps, False, None)
        return fmaps

    def train(self, eng, lib):
        fmaps = [torch.empty(s, device="cuda") for s in self.shapes(eng, B)]
        self.fwd(eng)(_rand((B, 1, self.T), 10), fmaps, True, None)
        d = [torch.ones(s, device="cuda") for s in self.shapes(eng, B + 1)]
        ptrs = (ctypes.c_void_p * len(d))(*[t.data_ptr() for t in d])
        flat = torch.zeros(eng.grad_layout()[None], device="cuda")
        call = lambda b: getattr(lib, self.entry + "_backward")(eng.handle, ptrs, None, flat.data_ptr(), b, self.T, None)      # noqa: E731
        return call(B), call(B + 1), (f"{self.entry}_backward: the engine holds the activations of a forward with B={B}, T={self.T}, "
                                      f"not B={B + 1}, T={self.T}")


class PeriodDisc(_Disc):
    T, entry = PD_T, "st_period_disc_train"

    def create(self):
        from stabletts_amd import _lib
        return _lib.Engine(*DIT, period_discriminator=PD)

    def weights(self, eng):
        return mpd.make_dp_state_dict(14)

    def shapes(self, eng, b):
        return eng.period_disc_fmap_shapes(b, PD_T, PD["period"])

    def fwd(self, eng):
        return eng.period_disc_forward


class ResolutionDisc(_Disc):
    T, entry = RD_T, "st_resolution_disc_train"

    def create(self):
        from stabletts_amd import _lib
        return _lib.Engine(*DIT, resolution_discriminator=RD)

    def weights(self, eng):
        return mrd.make_dr_state_dict(15)

    def shapes(self, eng, b):
        return eng.resolution_disc_fmap_shapes(b, RD_T)

    def fwd(self, eng):
        return eng.resolution_disc_forward


class Ffgan(Kind):
    repack = VOCODER

    def create(self):
        from stabletts_amd import _lib
        return _lib.Engine(*DIT, ffgan=_lib.ffgan_config_fields(FFGAN["backbone"], FFGAN["head"]))

    def weights(self, eng):
        return ffr.make_state_dict(FFGAN, ffr.SEED)

    def forward(self, eng):
        audio = torch.empty(B, T * FFGAN["head"]["hop_length"], device="cuda")
        eng.ffgan_forward(ffr.make_mel(B, T, FFGAN["backbone"]["input_channels"], ffr.MEL_SEED).float().cuda(), audio, None)
        return [audio]


KINDS = {"decoder": Decoder(), "text_encoder": TextEncoder(), "vocoder": Vocoder(), "style_encoder": StyleEncoder(),
         "duration_predictor": DurationPredictor(), "mel_extractor": MelExtractor(), "period_disc": PeriodDisc(),
         "resolution_disc": ResolutionDisc(), "ffgan": Ffgan()}
TRAINS_THROUGH_HELD_ACTIVATIONS = ("vocoder", "style_encoder", "duration_predictor", "period_disc", "resolution_disc")


def _load(kind, eng):
    eng.load_state_dict(_tensors(kind.weights(eng)))      # st_load_param of every parameter, then st_finalize


@pytest.mark.parametrize("name", list(KINDS))
def test_handle_lifecycle(name):
    from stabletts_amd import _lib
    kind = KINDS[name]
    eng = kind.create()
    lib = eng.lib
    try:
        eng.device_bytes()      # answers for a handle with nothing loaded; the count is checked below
        _load(kind, eng)
        first = [t.clone() for t in kind.forward(eng)]
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in first)
        held = eng.device_bytes()
        # a handle of another kind comes and goes
        other = KINDS["mel_extractor" if name != "mel_extractor" else "style_encoder"]
        guest = other.create()
        _load(other, guest)
        guest.close()
        eng.finalize()
        again = kind.forward(eng)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(again, first))
        assert eng.device_bytes() == held
        rc = lib.st_repack(eng.handle, None)
        if kind.repack is None:
            assert rc == _lib.ST_OK, lib.st_last_error(eng.handle).decode()
        else:
            assert (rc, lib.st_last_error(eng.handle).decode()) == (_lib.ST_ERR_UNSUPPORTED, kind.repack)
        assert (kind.train is not None) == (name in TRAINS_THROUGH_HELD_ACTIVATIONS)
        if kind.train is not None:
            ok, other_b, text = kind.train(eng, lib)
            assert ok == _lib.ST_OK, lib.st_last_error(eng.handle).decode()
            assert (other_b, lib.st_last_error(eng.handle).decode()) == (_lib.ST_ERR_STATE, text)
        torch.cuda.synchronize()
    finally:
        eng.close()
