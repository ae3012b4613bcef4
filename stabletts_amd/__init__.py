"""stabletts_amd -- MI355X (gfx950) native flow-matching mel decoder for StableTTS.

Public surface mirrors the reference's ``models/flow_matching.py``:

    from stabletts_amd.flow_matching import CFMDecoder

``install()`` registers that module as ``models.flow_matching`` so the reference's
``models/model.py:7`` (``from models.flow_matching import CFMDecoder``) picks it up unmodified;
``install(text_encoder=True)`` also registers ``stabletts_amd.text_encoder`` as ``models.text_encoder``
(``models/model.py:6``), the caller side of the path on the same block kernels;
``install(reference_encoder=True, duration_predictor=True)`` registers the fp32 ``MelStyleEncoder`` /
``DurationPredictor`` as ``models.reference_encoder`` / ``models.duration_predictor`` (``models/model.py:8-9``), inference-only;
with ``"train"`` instead of ``True`` they register subclasses that also train natively (``native_training = True``);
``install(monotonic_align=True)`` registers ``stabletts_amd.monotonic_align`` as ``monotonic_align`` (``models/model.py:5``),
so the reference's training ``forward`` imports and runs its alignment search on the device, without numba;
``install(audio=True)`` registers ``stabletts_amd.audio`` as ``utils.audio`` (``api.py:6,17``, ``preprocess.py:11``): the
native ``LogMelSpectrogram`` feature front end, which needs no torchaudio; ``install(audio="train")`` registers
``stabletts_amd.audio_train`` instead, whose spectrograms are also differentiable in the waveform (``native_training = True``),
for the Vocos multi-scale mel loss (``vocoders/vocos/models/loss.py:6``);
``install(vocoder=True)`` registers ``stabletts_amd.vocos`` as ``vocoders.vocos.models.model`` (``api.py:26-28``), inference-only;
``install(vocoder="train")`` registers ``stabletts_amd.vocos_train`` instead, whose ``Vocos`` also trains natively in fp32
(``vocoders/vocos/train.py:94``: the generator);
``install(ffgan=True)`` registers ``stabletts_amd.ffgan`` as ``vocoders.ffgan.model`` (``api.py:21-23``: the default vocoder,
``FireflyGANBaseWrapper``), inference-only like the reference (its ``operand_dtype="f16_split"`` / ``"bf16_split"`` carry every
MFMA operand as a hi + lo pair: the waveform at fp32 distance from float64, ``"f16_split"`` at 1.5 x the time of the default ``"f16"``);
``install(discriminator="train")`` rebinds ``MultiPeriodDiscriminator`` and ``DiscriminatorP`` of the user's own
``vocoders.vocos.models.discriminator`` (``vocoders/vocos/train.py:19,54``) to the native classes of ``stabletts_amd.discriminator``;
and ``install(resolution_discriminator="train")`` rebinds ``MultiResolutionDiscriminator`` and ``DiscriminatorR`` of that same
module (``vocoders/vocos/train.py:19,55``), which need no torchaudio; each keyword leaves the other pair of names as it is;
``install(gan_losses=True)`` rebinds ``feature_loss``, ``discriminator_loss`` and ``generator_loss`` of the user's own
``vocoders.vocos.models.loss`` (``vocoders/vocos/train.py:20``) to the fused ones of ``stabletts_amd.gan_loss`` and leaves the two
mel-loss classes of that module as they are;
``install(model=True)`` registers ``stabletts_amd.model`` as ``models.model`` (``train.py:18``, ``api.py``): a ``StableTTS`` built
from the native classes whose ``forward`` runs the alignment search, ``mu_y``, the prior and duration losses and their gradients
on the device (``alignment.align_and_losses``), so that the reference's ``train.py`` needs no edit and no other registration.
"""
import sys

__all__ = ["install", "CFMDecoder", "TextEncoder", "MelStyleEncoder", "DurationPredictor", "maximum_path", "LogMelSpectrogram", "StableTTS", "FireflyGANBase"]


def install(text_encoder=False, vocoder=False, reference_encoder=False, duration_predictor=False, monotonic_align=False,
            audio=False, discriminator=False, model=False, resolution_discriminator=False, gan_losses=False, ffgan=False):
    """Make ``models.flow_matching`` (and optionally ``models.text_encoder`` / ``vocoders.vocos.models.model`` /
    ``models.reference_encoder`` / ``models.duration_predictor`` / ``monotonic_align`` / ``utils.audio``) resolve to the native drop-ins
    (call before importing models.model / api.get_vocoder)."""
    from . import flow_matching
    sys.modules["models.flow_matching"] = flow_matching
    if text_encoder:
        from . import text_encoder as te
        sys.modules["models.text_encoder"] = te
    if vocoder == "train":                                       # Vocos with native_training = True: the generator of vocoders/vocos/train.py
        from . import vocos_train
        sys.modules["vocoders.vocos.models.model"] = vocos_train
    elif vocoder:
        from . import vocos
        sys.modules["vocoders.vocos.models.model"] = vocos      # api.py:26-28: from vocoders.vocos.models.model import Vocos
    if ffgan:
        from . import ffgan as fg
        sys.modules["vocoders.ffgan.model"] = fg                 # api.py:21-23: from vocoders.ffgan.model import FireflyGANBaseWrapper
    if reference_encoder == "train":                             # MelStyleEncoder with native_training = True
        from . import reference_encoder_train as re_
        sys.modules["models.reference_encoder"] = re_            # models/model.py:8
    elif reference_encoder:
        from . import reference_encoder as re_
        sys.modules["models.reference_encoder"] = re_
    if duration_predictor == "train":                            # DurationPredictor with native_training = True
        from . import duration_predictor_train as dp
        sys.modules["models.duration_predictor"] = dp            # models/model.py:9
    elif duration_predictor:
        from . import duration_predictor as dp
        sys.modules["models.duration_predictor"] = dp
    if monotonic_align:
        from . import monotonic_align as ma
        sys.modules["monotonic_align"] = ma                      # models/model.py:5
    if audio == "train":                                         # spectrograms with native_training = True
        from . import audio_train as au
        sys.modules["utils.audio"] = au                          # vocoders/vocos/models/loss.py:6 (the multi-scale mel loss)
    elif audio:
        from . import audio as au
        sys.modules["utils.audio"] = au                          # api.py:6, preprocess.py:11, vocoders/vocos/models/loss.py:6
    if discriminator:
        if discriminator != "train":
            raise ValueError('install(discriminator=...) takes "train": the discriminators exist for training only')
        import importlib
        from . import discriminator as nd
        try:                                                     # the user's module: its multi-resolution classes stay
            ref = importlib.import_module("vocoders.vocos.models.discriminator")
        except ImportError as exc:
            raise ImportError('install(discriminator="train") rebinds MultiPeriodDiscriminator and DiscriminatorP inside '
                              "vocoders.vocos.models.discriminator, which could not be imported (is the StableTTS checkout on "
                              f"sys.path, and are its own imports such as torchaudio installed?): {exc}") from exc
        ref.MultiPeriodDiscriminator = nd.MultiPeriodDiscriminator      # vocoders/vocos/train.py:19,54
        ref.DiscriminatorP = nd.DiscriminatorP
    if resolution_discriminator:
        if resolution_discriminator != "train":
            raise ValueError('install(resolution_discriminator=...) takes "train": the discriminators exist for training only')
        import importlib
        from . import discriminator as nd
        try:                                                     # the user's module: its multi-period classes stay
            ref = importlib.import_module("vocoders.vocos.models.discriminator")
        except ImportError as exc:
            raise ImportError('install(resolution_discriminator="train") rebinds MultiResolutionDiscriminator and DiscriminatorR inside '
                              "vocoders.vocos.models.discriminator, which could not be imported (is the StableTTS checkout on "
                              f"sys.path, and are its own imports such as torchaudio installed?): {exc}") from exc
        ref.MultiResolutionDiscriminator = nd.MultiResolutionDiscriminator      # vocoders/vocos/train.py:19,55
        ref.DiscriminatorR = nd.DiscriminatorR
    if gan_losses:
        import importlib
        from . import gan_loss as gl
        try:                                                     # the user's module: its two mel-loss classes stay
            ref = importlib.import_module("vocoders.vocos.models.loss")
        except ImportError as exc:
            raise ImportError("install(gan_losses=True) rebinds feature_loss, discriminator_loss and generator_loss inside "
                              "vocoders.vocos.models.loss, which could not be imported (is the StableTTS checkout on "
                              f"sys.path, and are its own imports such as torchaudio installed?): {exc}") from exc
        ref.feature_loss = gl.feature_loss                       # vocoders/vocos/train.py: the three loss lines of a step
        ref.discriminator_loss = gl.discriminator_loss
        ref.generator_loss = gl.generator_loss
    if model:
        from . import model as md
        sys.modules["models.model"] = md                         # train.py:18, api.py: from models.model import StableTTS
    return flow_matching


def __getattr__(name):
    if name == "CFMDecoder":
        from .flow_matching import CFMDecoder
        return CFMDecoder
    if name == "Vocos":
        from .vocos import Vocos
        return Vocos
    if name == "FireflyGANBase":
        from .ffgan import FireflyGANBase
        return FireflyGANBase
    if name == "TextEncoder":
        from .text_encoder import TextEncoder
        return TextEncoder
    if name == "MelStyleEncoder":
        from .reference_encoder import MelStyleEncoder
        return MelStyleEncoder
    if name == "DurationPredictor":
        from .duration_predictor import DurationPredictor
        return DurationPredictor
    if name == "LogMelSpectrogram":
        from .audio import LogMelSpectrogram
        return LogMelSpectrogram
    if name == "MultiPeriodDiscriminator":
        from .discriminator import MultiPeriodDiscriminator
        return MultiPeriodDiscriminator
    if name == "MultiResolutionDiscriminator":
        from .discriminator import MultiResolutionDiscriminator
        return MultiResolutionDiscriminator
    if name == "StableTTS":
        from .model import StableTTS
        return StableTTS
    if name == "maximum_path":
        from .monotonic_align import maximum_path
        return maximum_path
    raise AttributeError(name)
