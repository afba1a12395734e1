"""Case builders shared by test_annotate_host.py and test_gpu_annotate.py: the golden fixture, the head-on box whose
visibility is known by construction, the five-pose scene of the device parity tests and the numpy restatements."""
import functools
import os

import numpy as np

import raster_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT, IN_IMAGE, SELF, SCENE, KNOWN = 1, 2, 4, 8, 16


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "annot.npz"))
    return {k: g[k] for k in g.files}


def true_projection(poses, pts, K):
    """numpy float64 projection [P, n, 2] and depth [P, n] of model points."""
    poses = np.asarray(poses, dtype=np.float64)
    X = np.einsum("pij,nj->pni", poses[:, :3, :3], pts) + poses[:, None, :3, 3]
    u = (K[0, 0] * X[..., 0] + K[0, 1] * X[..., 1]) / X[..., 2] + K[0, 2]
    v = K[1, 1] * X[..., 1] / X[..., 2] + K[1, 2]
    return np.stack([u, v], axis=-1), X[..., 2]


def box_case():
    """A 10 cm cube seen head-on from 0.5 m in raster_common's 64 x 48 camera, and 18 key points: 0-4 the front face's
    centre and corners (visible), 5-9 the back face's (hidden behind the front face: they project inside it), 10-13 the
    side faces' centres (hidden likewise), 14 a point beside the object (an uncovered pixel), 15 a point that projects
    outside the image, 16 a point behind the camera, 17 a point nearer than ``near``."""
    v, f = rc.box()
    v = v * 0.1
    pose = np.hstack([np.eye(3), [[0.0], [0.0], [0.5]]])[None]
    h = 0.05
    corners = [(x, y) for x in (-h, h) for y in (-h, h)]
    kp = [(0, 0, -h)] + [(x, y, -h) for x, y in corners] + [(0, 0, h)] + [(x, y, h) for x, y in corners]
    kp += [(-h, 0, 0), (h, 0, 0), (0, -h, 0), (0, h, 0), (0.2, 0.0, 0.0), (0.5, 0.0, 0.0), (0.0, 0.0, -0.6), (0.0, 0.0, -0.495)]
    return v, f, pose, np.array(kp, dtype=np.float64)


def box_from_mask(mask):
    """get_bbox_from_mask's (xmin, xmax, ymin, ymax), -1 x4 for an empty mask."""
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return [-1, -1, -1, -1]
    return [int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())]


def mask_boxes_np(depth, K, scene, index, delta, c=0.0):
    """numpy restatement of mask_boxes through metrics.vsd_masks."""
    from betapose_amd import metrics
    boxes, counts = [], []
    for p in range(len(depth)):
        full = depth[p] > 0
        vis = full if scene is None else metrics.vsd_masks(scene[index[p]], depth[p], depth[p], K, delta, c)["visib_gt"]
        boxes.append([box_from_mask(full), box_from_mask(vis)])
        counts.append([int(full.sum()), int(vis.sum())])
    return np.array(boxes, dtype=np.int32), np.array(counts, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def parity_scene(H, W):
    """The device parity scene at H x W: an icosphere of 5 cm radius at P = 5 poses -- two in view, one out of view to
    the right (an empty render), one centred on the left image border (cut), one behind the camera (empty, not FRONT)
    -- Kp = 7 points on its surface, n = 500 random vertices for the vertex boxes and T = 2 scene depth images built
    from the renders of poses 0 and 3: a wall behind, an occluder plane over the left part, a band of missing depth."""
    from betapose_amd import metrics
    f = 0.9 * W
    K = np.array([[f, 0.3, (W - 1) / 2.0], [0.0, f * 1.01, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    v, faces = rc.icosphere()
    v = v * 0.05
    rng = np.random.default_rng(11)
    poses = np.tile(np.eye(4)[:3], (5, 1, 1))
    for p in range(5):
        poses[p, :, :3] = rc.rand_rot(rng)
    poses[0, :, 3] = [0.01, -0.005, 0.25]
    poses[1, :, 3] = [-0.03, 0.02, 0.35]
    poses[2, :, 3] = [5.0, 0.0, 0.6]
    poses[3, :, 3] = [-K[0, 2] / K[0, 0] * 0.3, 0.01, 0.3]
    poses[4, :, 3] = [0.0, 0.0, -0.3]
    kp = rng.normal(size=(7, 3))
    kp = kp / np.linalg.norm(kp, axis=1, keepdims=True) * 0.05
    cloud = rng.normal(size=(500, 3)) * 0.03
    depth, _ = metrics.render_depth(poses, v, faces, K, (H, W))
    assert (depth[0] > 0).any() and not (depth[2] > 0).any() and not (depth[4] > 0).any()
    assert (depth[3][:, 0] > 0).any()                                   # cut by the left border
    scene = np.zeros((2, H, W), np.float32)
    for t, p in enumerate((0, 3)):
        s = np.where(depth[p] > 0, depth[p].astype(np.float64), 0.6)
        s[:, :W // 2 - 2 + 3 * t] = np.minimum(s[:, :W // 2 - 2 + 3 * t], poses[p, 2, 3] - 0.1)
        s[H // 2 - 1 + t:H // 2 + 2 + t, :] = 0.0
        scene[t] = s.astype(np.float32)
    index = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    for a in (depth, scene, index, poses, kp, cloud):
        a.setflags(write=False)
    return {"K": K, "v": v, "faces": faces, "poses": poses, "kp": kp, "cloud": cloud, "depth": depth, "scene": scene,
            "index": index, "size": (H, W)}


def target_case(resH, resW):
    """B = 3 samples x 6 parts at inp = 4 x res: interior parts, Gaussians clipped by each border, a part outside its
    window and a part with x <= 0."""
    inpH, inpW = 4 * resH, 4 * resW
    ul = np.array([[10, 20], [0, 0], [30, 5]], dtype=np.float32)
    br = ul + np.array([[inpW, inpH], [inpW * 2, inpH], [inpW, inpH * 2]], dtype=np.float32)
    parts = np.zeros((3, 6, 2))
    for b in range(3):
        w, h = br[b] - ul[b]
        parts[b] = ul[b] + np.array([[0.5 * w, 0.45 * h], [2.3, 0.5 * h], [w - 2.2, h - 2.4], [0.4 * w, 1.7],
                                     [-5.0, 0.5 * h], [0.37 * w, 0.61 * h]])
    parts[1, 4] = [0.0, 50.0]                                           # x <= 0 (and on the window's edge)
    return parts, ul, br, (inpH, inpW), (resH, resW)
