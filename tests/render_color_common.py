"""What test_render_color_host.py and test_gpu_render_color.py share: seeded vertex colours, an independent numpy f64
colour ray caster (Moller-Trumbore nearest hit with its face and barycentrics, then the shading formula of DESIGN.md 3.5
written out in numpy), the scenes of every test, and ``CASES``: name -> function(device) -> tuple of arrays, the calls the
GPU test repeats on the device and compares byte for byte with the host's.  The cases of ``SIZE_FREE`` also take an image
size, function(device, size) (default raster_common.SIZE; the camera is raster_common.camera(size))."""
import functools

import numpy as np

import raster_common as rc

H, W, K = rc.H, rc.W, rc.K
LIGHTS = [(0.0, 0.0, 0.0), (0.3, -0.2, 0.0)]
RED, BLUE = (255, 0, 0), (0, 0, 255)


def colors_for(n, seed=11):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3), dtype=np.uint8)


def ray_cast_color(pose, v, f, colors, c, ambient, light, size=rc.SIZE):
    """(color [H, W, 3] float64 before rounding is applied as floor(x + 0.5) clipped to 255, hit [H, W] bool)."""
    (H, W), K = size, rc.camera(size)
    X = rc.camera_vertices(pose, v)
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([(xs + c - K[0, 2]) / K[0, 0], (ys + c - K[1, 2]) / K[1, 1], np.ones((H, W))], axis=-1).reshape(-1, 1, 3)
    v0, e1, e2 = X[f[:, 0]][None], (X[f[:, 1]] - X[f[:, 0]])[None], (X[f[:, 2]] - X[f[:, 0]])[None]
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = -v0
        u = (tv * pv).sum(-1) * inv
        qv = np.cross(tv, e1)
        w = (d * qv).sum(-1) * inv
        t = (e2 * qv).sum(-1) * inv
    hit = (np.abs(det) > 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)
    t = np.where(hit, t, np.inf)
    face = t.argmin(axis=1)
    px = np.arange(H * W)
    tn, un, wn = t[px, face], u[px, face], w[px, face]
    any_hit = np.isfinite(tn)
    tn = np.where(any_hit, tn, 1.0)
    point = tn[:, None] * d[:, 0, :]
    col = colors.astype(np.float64)
    base = ((1.0 - un - wn)[:, None] * col[f[face, 0]] + un[:, None] * col[f[face, 1]] + wn[:, None] * col[f[face, 2]])
    n = np.cross(e1[0][face], e2[0][face])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where((n * point).sum(-1, keepdims=True) > 0, -n, n)
    to_light = np.asarray(light, dtype=np.float64)[None] - point
    length = np.linalg.norm(to_light, axis=1, keepdims=True)
    to_light = np.where(length > 0, to_light / np.where(length > 0, length, 1.0), 0.0)
    light_w = np.minimum(ambient + 0.5 * np.maximum((to_light * n).sum(-1), 0.0), 1.0)
    out = np.minimum(np.floor(light_w[:, None] * base + 0.5), 255.0)
    return np.where(any_hit[:, None], out, 0.0).reshape(H, W, 3), any_hit.reshape(H, W)


def quad(c=0.0, cam=K):
    """The fronto-parallel rectangle of test_shared_edge_and_top_left_rule: pixels 10 .. 19 x 5 .. 14 at depth 2."""
    z = 2.0
    v = np.array([[(u + c - cam[0, 2]) / cam[0, 0] * z, (w + c - cam[1, 2]) / cam[1, 1] * z, z]
                  for u, w in [(10, 5), (20, 5), (20, 15), (10, 15)]])
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


QUAD_COLOR = np.tile(np.array([200, 100, 50], np.uint8), (4, 1))
K_AXIS = K.copy()
K_AXIS[0, 2], K_AXIS[1, 2] = 14.0, 9.0        # the centre of pixel (14, 9) lies on the optical axis (pixel_center 0)
EYE = np.eye(4)[None, :3]


def coincident(order):
    """Two triangles on the same three points, one red, one blue, in the given face order."""
    tri = np.array([[-0.5, -0.4, 2.0], [0.6, -0.3, 2.0], [0.0, 0.5, 2.0]])
    v = np.concatenate([tri, tri])
    col = np.array([RED] * 3 + [BLUE] * 3, np.uint8)
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    return v, f[list(order)], col


def two_mesh_scene():
    """The icosphere and, beside it and further back, the box, each at its own pose: as two meshes drawn one after the
    other, and as ONE mesh (the box's vertices moved into the icosphere's frame) at the icosphere's pose."""
    sv, sf = rc.icosphere()
    bv, bf = rc.box()
    ps = rc.poses_for("icosphere")[0]
    pb = np.hstack([rc.rand_rot(np.random.default_rng(3)), [[0.45], [0.2], [float(ps[2, 3]) + 0.37]]])
    # box vertices in the icosphere's object frame: R_s^T (R_b x + t_b - t_s)
    moved = (rc.camera_vertices(pb, bv) - ps[:, 3]) @ ps[:, :3]
    return (sv, sf, colors_for(len(sv), 1), ps), (bv, bf, colors_for(len(bv), 2), pb), \
        (np.concatenate([sv, moved]), np.concatenate([sf, bf + len(sv)]).astype(np.int32))


def unit_box_corners():
    from betapose_amd import metrics
    return metrics.box_corners(rc.box()[0])


def guard_image(fill=9, pad=3):
    """A [1, H, W, 3] image that is a view into the middle rows of a larger sentinel array (rows are contiguous, so the
    guard rows lie right before and after the image in memory)."""
    big = np.full((1 + 2 * pad, H, W, 3), 77, np.uint8)
    big[pad] = fill
    return big, pad


def box_pose(x=0.0, y=0.0, z=3.0, rot=None):
    return np.hstack([np.eye(3) if rot is None else rot, [[x], [y], [z]]])[None]


BOX_POSES = {
    "frontal": box_pose(z=3.0),
    "rotated": box_pose(0.1, -0.05, 2.5, rc.rand_rot(np.random.default_rng(4))),
    "crosses_near": box_pose(z=0.9),                       # drawn with near = 0.5: the front corners (z = 0.4) lie behind it
    "outside": box_pose(x=40.0, z=4.0),
    "behind": box_pose(z=-3.0),
    "closeup": box_pose(0.2, 0.1, 0.9, rc.rand_rot(np.random.default_rng(6))),   # edges leave the image on all sides
}


def _mesh_case(name, c):
    def run(device, size=rc.SIZE):
        from betapose_amd import metrics
        v, f = rc.MESHES[name]()
        return metrics.render_color(rc.poses_for(name, size=size), v, f, colors_for(len(v)), rc.camera(size), size, device,
                                    pixel_center=c, light=LIGHTS[1])
    return run


def _edge_case(name):
    def run(device, size=rc.SIZE):
        from betapose_amd import metrics
        v, f, pose, near = rc.edge_cases(size)[name]
        return metrics.render_color(pose[None], v, f, colors_for(len(v)), rc.camera(size), size, device, near=near)
    return run


def _quad_case(ambient, cam):
    def run(device):
        from betapose_amd import metrics
        v, f = quad(0.0, cam)
        return metrics.render_color(EYE, v, f, QUAD_COLOR, cam, (H, W), device, ambient=ambient)
    return run


def _tie_case(order, poses=1):
    def run(device, size=rc.SIZE):
        from betapose_amd import metrics
        v, f, col = coincident(order)
        return metrics.render_color(np.repeat(EYE, poses, axis=0), v, f, col, rc.camera(size), size, device,
                                    image_index=np.zeros(poses, np.int32), images=1, ambient=1.0)
    return run


def _index_case(index, images):
    def run(device, size=rc.SIZE):
        from betapose_amd import metrics
        v, f = rc.torus()
        return metrics.render_color(rc.poses_for("torus", size=size)[:2], v, f, colors_for(len(v)), rc.camera(size), size, device,
                                    image_index=index, images=images)
    return run


def _accumulate_case(device, size=rc.SIZE):
    from betapose_amd import metrics
    (sv, sf, sc, ps), (bv, bf, bc, pb), _ = two_mesh_scene()
    first = metrics.render_color(ps[None], sv, sf, sc, rc.camera(size), size, device)
    second = metrics.render_color(pb[None], bv, bf, bc, rc.camera(size), size, device, into=first[:2])
    return first + second


def _boxes_case(names):
    def run(device, size=rc.SIZE):
        from betapose_amd import metrics
        poses = np.concatenate([BOX_POSES[n] for n in names])
        index = np.minimum(np.arange(len(poses)) // 2, 1).astype(np.int32) if len(poses) > 1 else None
        images = 2 if len(poses) > 1 else 1
        base = np.full((images,) + tuple(size) + (3,), 9, np.uint8)
        return (metrics.draw_boxes(base, poses, unit_box_corners(), rc.camera(size), None, device, index, near=0.5),)
    return run


def overlay_inputs(size=rc.SIZE):
    H, W = size
    rng = np.random.default_rng(17)
    frames = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    color = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    depth = np.where(rng.random((2, H, W)) < 0.4, rng.random((2, H, W)) + 0.5, 0.0).astype(np.float32)
    return frames, color, depth


def _overlay_case(alpha):
    def run(device, size=rc.SIZE):
        from betapose_amd import metrics
        return (metrics.overlay(*overlay_inputs(size), alpha=alpha, device=device),)
    return run


CASES = {}
for _name in ("icosphere", "torus", "box"):
    for _c in (0.0, 0.5):
        CASES["mesh-%s-%.1f" % (_name, _c)] = _mesh_case(_name, _c)
for _name in ("box_closeup", "half_outside", "outside", "behind_near"):
    CASES["edge-" + _name] = _edge_case(_name)
CASES["quad-ambient1"] = _quad_case(1.0, K)
CASES["quad-on-axis"] = _quad_case(0.5, K_AXIS)
CASES["tie-red-blue"] = _tie_case((0, 1))
CASES["tie-blue-red"] = _tie_case((1, 0))
CASES["tie-two-poses"] = _tie_case((0, 1), poses=2)
CASES["index-00"] = _index_case([0, 0], 1)
CASES["index-01"] = _index_case([0, 1], 2)
CASES["accumulate"] = _accumulate_case
CASES["boxes-frontal"] = _boxes_case(["frontal"])
CASES["boxes-crosses-near"] = _boxes_case(["crosses_near"])
CASES["boxes-nothing"] = _boxes_case(["outside", "behind"])
CASES["boxes-many"] = _boxes_case(["frontal", "rotated", "closeup", "crosses_near", "outside"])
for _alpha in (0, 128, 256):
    CASES["overlay-%d" % _alpha] = _overlay_case(_alpha)


# the cases that take an image size: all but the quads, whose expectations are written in pixel coordinates
SIZE_FREE = sorted(n for n in CASES if not n.startswith("quad-"))


@functools.lru_cache(maxsize=None)
def host(name, size=rc.SIZE):
    """The host twin's result of a case, computed once per session and read-only."""
    out = CASES[name](None) if tuple(size) == rc.SIZE else CASES[name](None, size)
    for a in out:
        a.setflags(write=False)
    return out
