from .model import get_model, use_device_norm  # noqa: F401
