from .deepfm import DeepFMTrainer  # noqa: F401
from .ffm import FFMTrainer, ffm_batch  # noqa: F401
from .fm import FMTrainer  # noqa: F401
