"""Meshes, poses, the independent ray caster and the edge cases shared by test_raster_host.py and test_gpu_raster.py.

Everything that depends on the camera takes ``size=(H, W)``; the camera of a size is ``camera(size)``.  ``SIZES`` are the
image shapes the raster, VSD, ICP and colour tests run at, and what each opens in the kernels:
  (48, 64)   3 072 px, the shape of every test before the sizes: W is the wave width and divides the 256-thread block (a
             lane keeps one column, ``i / W`` is a shift), one VSD slice (vsd.hip VSD_PIX = 4 096), two whole ICP slices
             (icp.hip ICP_PIX = 2 048).
  (75, 113)  8 475 px: W is an odd prime above the wave width, so a lane's column changes from pixel to pixel, the border
             test falls on other lanes in every row and ``i / W`` is a division; three VSD slices (4 096 + 4 096 + 283,
             the first boundary inside row 36 at x = 28) and five ICP slices (4 x 2 048 + 283).
  (129, 67)  8 643 px: H > W, W three past a wave; three VSD and five ICP slices, the last of 451 pixels.
A size opens a slice only for a scene that puts pixels there.  The random poses keep their objects round the middle of
the image, so the last slice of either kind stays empty in them: the VSD rectangles of test_gpu_raster.py and the
frame-filling icp_common.closeup_scene are what feed it.
``MANY`` poses on a ``MANY_SIZE`` image are two more than a grid has columns (65 535): the ``q += gridDim.y`` loops over
poses and pairs iterate twice, and MANY * 256 elements are more than the 65 535 blocks of raster_finish_kernel hold."""
import functools

import numpy as np

SIZE = (48, 64)
SIZES = [(48, 64), (75, 113), (129, 67)]
MANY, MANY_SIZE, MANY_CYCLE = 65538, (16, 16), 7


def camera(size=SIZE):
    """The camera matrix of an image size: f = 60 px at 48 x 64 and in proportion to the tighter side elsewhere, the
    principal point in the middle of the image."""
    H, W = size
    f = 60 * min(W / 64, H / 48)
    return np.array([[f, 0.0, (W - 1) / 2], [0.0, f, (H - 1) / 2], [0.0, 0.0, 1.0]])


H, W = SIZE
K = camera(SIZE)


def rand_rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def icosphere():
    """An icosahedron subdivided once: 42 vertices on the unit sphere, 80 faces (one full wave of triangles plus 16)."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    mid = {}

    def midpoint(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            m = v[a] + v[b]
            v.append(m / np.linalg.norm(m))
            mid[key] = len(v) - 1
        return mid[key]
    out = []
    for a, b, c in f:
        ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return np.array(v), np.array(out, dtype=np.int32)


def torus(nu=16, nv=8, R=1.0, r=0.4):
    """nu x nv quads split in two: 128 vertices, 256 faces; it occludes itself at most poses."""
    v, f = [], []
    for i in range(nu):
        for j in range(nv):
            a, b = 2 * np.pi * i / nu, 2 * np.pi * j / nv
            v.append(((R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)))
    for i in range(nu):
        for j in range(nv):
            p00, p10 = i * nv + j, ((i + 1) % nu) * nv + j
            p01, p11 = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
            f += [(p00, p10, p11), (p00, p11, p01)]
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int32)


def box():
    """The unit cube about the origin: 8 vertices, 12 faces."""
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], dtype=np.float64)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    return v, f


MESHES = {"icosphere": icosphere, "torus": torus, "box": box}
# seed and distance range (in object diameters) of each mesh's random poses.  With an edge band of 2^-7 px the share of
# ambiguous pixels grows with the edge length per covered pixel, so the finely triangulated torus (256 faces, both sides
# project) sits closer than the other two; seeds checked on the CPU to keep every image under the 5 % cap
SEEDS = {"icosphere": 2, "torus": 8, "box": 2}
RANGES = {"icosphere": (1.8, 2.6), "torus": (1.3, 1.7), "box": (1.8, 2.6)}


def diameter(v):
    return float(np.sqrt(((v[:, None, :] - v[None, :, :]) ** 2).sum(axis=2)).max())


def poses_for(name, count=4, size=SIZE):
    """Seeded random rotations at RANGES[name] diameters: the object spans 23 .. 33 px of the 64 x 48 image (the torus
    35 .. 46 px, partly cut by the border), a few pixels off the principal point.  The poses are the same at every
    ``size``; the camera's focal length grows with it, so the object fills the same share of the tighter side."""
    v, _ = MESHES[name]()
    d = diameter(v)
    rng = np.random.default_rng(SEEDS[name])
    out = np.tile(np.eye(4)[:3], (count, 1, 1))
    for p in range(count):
        z = d * rng.uniform(*RANGES[name])
        out[p, :, :3] = rand_rot(rng)
        out[p, :, 3] = [rng.uniform(-4, 4) * z / 60.0, rng.uniform(-3, 3) * z / 60.0, z]
    return out


def camera_vertices(pose, v):
    return v @ pose[:3, :3].T + pose[:3, 3]


def ray_cast(pose, v, f, c, size=SIZE):
    """Nearest hit of every pixel's ray with every triangle (Moller-Trumbore, numpy f64): depth z [H, W], 0 = no hit."""
    (H, W), K = size, camera(size)
    X = camera_vertices(pose, v)
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([(xs + c - K[0, 2]) / K[0, 0], (ys + c - K[1, 2]) / K[1, 1], np.ones((H, W))], axis=-1).reshape(-1, 1, 3)
    v0, e1, e2 = X[f[:, 0]][None], (X[f[:, 1]] - X[f[:, 0]])[None], (X[f[:, 2]] - X[f[:, 0]])[None]
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = -v0                                  # the ray starts at the camera centre
        u = (tv * pv).sum(-1) * inv
        qv = np.cross(tv, e1)
        w = (d * qv).sum(-1) * inv
        t = (e2 * qv).sum(-1) * inv
        hit = (np.abs(det) > 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)    # (det == 0: inf - inf, and no hit)
    t = np.where(hit, t, np.inf).min(axis=1)      # d has z = 1, so t is the depth
    return np.where(np.isfinite(t), t, 0.0).reshape(H, W)


def ambiguous(pose, v, f, c, tol=2.0 ** -7, size=SIZE):
    """Pixels whose centre lies within ``tol`` px of a projected triangle edge (f64, unsnapped)."""
    (H, W), K = size, camera(size)
    X = camera_vertices(pose, v)
    uv = np.stack([K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2] - c, K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2] - c], axis=1)
    a = np.concatenate([uv[f[:, 0]], uv[f[:, 1]], uv[f[:, 2]]])[None]
    b = np.concatenate([uv[f[:, 1]], uv[f[:, 2]], uv[f[:, 0]]])[None]
    ys, xs = np.mgrid[0:H, 0:W]
    p = np.stack([xs, ys], axis=-1).reshape(-1, 1, 2).astype(np.float64)
    ab = b - a
    den = (ab * ab).sum(-1)
    s = np.clip(((p - a) * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
    dist = np.sqrt((((a + s[..., None] * ab) - p) ** 2).sum(-1))
    return (dist.min(axis=1) < tol).reshape(H, W)


def edge_cases(size=SIZE):
    """name -> (vertices, faces, pose [3, 4], near): the situations beyond the random poses."""
    K = camera(size)
    bv, bf = box()
    sv, sf = icosphere()
    rot = rand_rot(np.random.default_rng(5))
    tilt = np.array([[np.cos(0.1), 0, np.sin(0.1)], [0, 1, 0], [-np.sin(0.1), 0, np.cos(0.1)]])
    cases = {}
    # 12 triangles, each box far above the cooperative threshold: nearly the whole frame is covered
    cases["box_closeup"] = (bv, bf, np.hstack([tilt, [[0.02], [-0.01], [0.95]]]), 0.01)
    cases["half_outside"] = (sv, sf, np.hstack([rot, [[-K[0, 2] * 4.0 / K[0, 0]], [0.3], [4.0]]]), 0.01)   # centre at x = 0
    cases["outside"] = (sv, sf, np.hstack([rot, [[40.0], [0.0], [4.0]]]), 0.01)
    # the cube straddles the camera plane: triangles with a vertex behind `near` are dropped and counted
    cases["behind_near"] = (bv, bf, np.hstack([rot, [[0.1], [0.05], [0.3]]]), 0.01)
    return cases


def pixel_quad(corners, depths, size=SIZE, c=0.0):
    """(vertices [4, 3], faces [2, 3]) of the quad whose corners project to the pixel coordinates ``corners`` (four
    (u, v) in pixel-index coordinates, in order round the quad) at the camera-space depths ``depths``, drawn at the
    identity pose and split along the diagonal from corner 0 to corner 2."""
    K = camera(size)
    v = np.array([[(u + c - K[0, 2]) / K[0, 0] * z, (w + c - K[1, 2]) / K[1, 1] * z, z] for (u, w), z in zip(corners, depths)])
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def pixel_rect(x0, y0, x1, y1, z=2.0, size=SIZE):
    """The fronto-parallel rectangle that covers exactly the pixels x0 .. x1 - 1 by y0 .. y1 - 1 (top-left rule)."""
    return pixel_quad([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], [z] * 4, size)


# The large-coordinate quad: every vertex projects between 10 000 and 16 000 px from the origin on both axes (snapped:
# up to 2^22 in 1/256 px), so an edge function multiplies differences of up to 2^23 and reaches about 2^44 -- far beyond
# 32 bits -- while the quad covers the whole 113 x 75 image and its diagonal from corner 0 to corner 2 crosses it from
# (0, 14.6) to (59.4, 74): both triangles own a part of the image, and a wrong high half of a product moves the diagonal.
# The depths differ, so the two planes do too.
BIG_QUAD_CORNERS = [(-12000.0, -11990.0), (15000.0, -13000.0), (14000.0, 14020.0), (-15000.0, 12000.0)]
BIG_QUAD_DEPTHS = [2.0, 2.5, 3.0, 2.25]
BIG_QUAD_SIZE = (75, 113)


def big_quad(out_of_range=False):
    """The large-coordinate quad; ``out_of_range``: corner 2, which both triangles share, moved to u = 16 390 px, just
    past the +-16 384 px that rs_project accepts."""
    corners = list(BIG_QUAD_CORNERS)
    if out_of_range:
        corners[2] = (16390.0, corners[2][1])
    return pixel_quad(corners, BIG_QUAD_DEPTHS, BIG_QUAD_SIZE)


def many_poses(count=MANY_CYCLE):
    """``count`` seeded poses of the box that fill a good part of the MANY_SIZE image (the box spans 7 .. 12 of its 16
    pixels), for the tests that cycle through them MANY times."""
    rng = np.random.default_rng(41)
    out = np.tile(np.eye(4)[:3], (count, 1, 1))
    for p in range(count):
        out[p, :, :3] = rand_rot(rng)
        out[p, :, 3] = [rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(1.9, 2.4)]
    return out


@functools.lru_cache(maxsize=None)
def host_render(name, c, size=SIZE):
    """(depth [P, H, W], skipped [P]) of the four random poses of a mesh on the host, computed once per session."""
    from betapose_amd import metrics
    v, f = MESHES[name]()
    depth, skipped = metrics.render_depth(poses_for(name, size=size), v, f, camera(size), size, None, c)
    depth.setflags(write=False)
    skipped.setflags(write=False)
    return depth, skipped


def vsd_margin(gt, est, v, f, test, index, d, size=SIZE, depth_scale=0.001):
    """The smallest distance of any pixel of these pairs from a decision of the VSD definition, from the host's
    intermediates: |dist - dist_test - delta| on the rendered pixels of either render and |rel - tau| on the
    intersection.  The parity tests' precondition is that it exceeds 1e-9, so a last-bit difference in a distance could
    not move a count."""
    from betapose_amd import metrics
    K = camera(size)
    dg = metrics.render_depth(gt, v, f, K, size)[0]
    de = metrics.render_depth(est, v, f, K, size)[0]
    worst = np.inf
    for p in range(len(gt)):
        m = metrics.vsd_masks(test[index[p]].astype(np.float64) * depth_scale, dg[p], de[p], K, metrics.BOP_VSD_DELTA)
        for name in ("dist_gt", "dist_est"):
            on = m[name] > 0
            if on.any():
                worst = min(worst, np.abs((m[name] - m["dist_test"])[on] - metrics.BOP_VSD_DELTA).min())
        if m["inter"].any():
            rel = np.abs(m["dist_gt"] - m["dist_est"])[m["inter"]] / d
            worst = min(worst, np.abs(rel[:, None] - np.asarray(metrics.BOP_VSD_TAUS)[None]).min())
    return worst


def vsd_scene(seed=21, size=SIZE):
    """The VSD parity scene: the torus and the icosphere are scored in one mesh (the icosphere beside the torus), P = 5
    pairs over T = 2 test images.  The estimates are off by 0 .. 10 % of the diameter; a test image is the render of its
    first pair's ground truth with an occluder plane over the left part and a band of zeros (missing depth), both placed
    in proportion to the image."""
    from betapose_amd import metrics
    (H, W), K = size, camera(size)
    tv, tf = torus()
    sv, sf = icosphere()
    v = np.concatenate([tv, sv * 0.6 + [0.0, 0.0, 1.2]])
    f = np.concatenate([tf, sf + len(tv)]).astype(np.int32)
    v = v * (0.1 / diameter(v))                   # a 10 cm object, poses in metres
    d = diameter(v)
    rng = np.random.default_rng(seed)
    P, T = 5, 2
    gt = np.tile(np.eye(4)[:3], (P, 1, 1))
    est = gt.copy()
    index = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    base = [None] * T
    for p in range(P):
        t = int(index[p])
        if base[t] is None:
            z = d * rng.uniform(1.8, 2.4)
            base[t] = (rand_rot(rng), np.array([rng.uniform(-3, 3) * z / 60.0, rng.uniform(-2, 2) * z / 60.0, z]))
        gt[p, :, :3], gt[p, :, 3] = base[t]
        a = rng.normal(size=3) * 0.04
        th = np.linalg.norm(a)
        A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / th
        est[p, :, :3] = gt[p, :, :3] @ (np.eye(3) + np.sin(th) * A + (1 - np.cos(th)) * A @ A)
        shift = rng.normal(size=3)
        est[p, :, 3] = gt[p, :, 3] + shift / np.linalg.norm(shift) * d * 0.1 * p / (P - 1)
    test = np.zeros((T, H, W), dtype=np.uint16)
    for t in range(T):
        p = int(np.argmax(index == t))
        depth = metrics.render_depth(gt[p:p + 1], v, f, K, (H, W))[0][0].astype(np.float64)
        scene = np.where(depth > 0, depth, 0.6)                       # a back wall behind the object
        edge, top = (26 + 4 * t) * W // 64, (20 + 3 * t) * H // 48
        scene[:, :edge] = np.minimum(scene[:, :edge], float(gt[p, 2, 3]) - 0.08)   # the occluder plane
        scene[top:top + 3 * H // 48, :] = 0.0                          # missing depth
        test[t] = np.round(scene * 1000.0).astype(np.uint16)
    return v, f, gt, est, test, index, d
