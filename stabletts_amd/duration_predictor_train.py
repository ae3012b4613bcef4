"""``models.duration_predictor`` for native training (``install(duration_predictor="train")``): the same module as
``duration_predictor`` -- constructor, checkpoint keys, inference path, ``duration_loss`` -- but ``DurationPredictor`` opts in
to native training (``native_training = True``): under autograd it runs st_duration_predictor_train_forward / _backward."""
from .duration_predictor import DurationPredictor as _DurationPredictor
from .duration_predictor import duration_loss  # noqa: F401  (models/model.py:9)


class DurationPredictor(_DurationPredictor):
    native_training = True
