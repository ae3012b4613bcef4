"""``utils.audio`` for Vocos training (``install(audio="train")``): the same module as ``audio`` -- constructors, state_dict keys,
inference path -- but ``LinearSpectrogram`` and ``LogMelSpectrogram`` opt in to native training (``native_training = True``):
under autograd, on a waveform that requires grad, they run the native forward and ``backward`` runs st_mel_backward instead of
raising.  vocoders/vocos/models/loss.py:6 imports ``LogMelSpectrogram`` from here for the multi-scale mel loss."""
from .audio import MelScale, frames, load_and_resample_audio, melscale_fbanks  # noqa: F401  (the names of audio)
from .audio import Resample, load_and_resample_wav, resample, resample_ragged, resample_table  # noqa: F401
from .audio import LinearSpectrogram as _LinearSpectrogram
from .audio import LogMelSpectrogram as _LogMelSpectrogram


class LinearSpectrogram(_LinearSpectrogram):
    native_training = True


class LogMelSpectrogram(_LogMelSpectrogram):
    native_training = True
