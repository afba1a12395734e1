"""``from utils.utils import pnp`` / ``draw_detections_3D``."""
from betapose_amd.ops import solve_pnp as pnp  # noqa: F401
from betapose_amd.renderer import draw_detections_3D, draw_poses  # noqa: F401
