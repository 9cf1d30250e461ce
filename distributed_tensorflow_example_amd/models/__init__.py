from .fm import FMTrainer  # noqa: F401
