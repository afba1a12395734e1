"""``from utils.utils import pnp`` / ``draw_detections_3D`` / ``verify_6D_poses``."""
from betapose_amd.ops import solve_pnp as pnp  # noqa: F401
from betapose_amd.renderer import draw_detections_3D, draw_poses, verify_6D_poses  # noqa: F401
