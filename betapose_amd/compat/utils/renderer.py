"""``from utils.renderer import Renderer``."""
from betapose_amd.renderer import Renderer  # noqa: F401

__all__ = ["Renderer"]
