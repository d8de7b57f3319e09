from src.losses.antibiasloss import AntibiasLoss  # noqa: F401
from src.losses.vggloss import VGGLoss  # noqa: F401
