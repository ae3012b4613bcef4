"""``models.reference_encoder`` for native training (``install(reference_encoder="train")``): the same module as
``reference_encoder`` -- constructor, checkpoint keys, inference path -- but ``MelStyleEncoder`` opts in to native training
(``native_training = True``): under autograd it runs st_style_encoder_train_forward / _backward instead of raising."""
from .reference_encoder import Conv1dGLU  # noqa: F401  (models/model.py:8 imports the module; the reference exports it)
from .reference_encoder import MelStyleEncoder as _MelStyleEncoder


class MelStyleEncoder(_MelStyleEncoder):
    native_training = True
