"""The depth refinement's definition restated in numpy, and the scenes shared by test_icp_host.py and test_gpu_icp.py.

``normal_equations_np`` and ``refine_np`` are written from the definition's text (the docstring of
metrics.refine_poses_depth), not from csrc/icp_math.inc: whole-image array expressions, numpy's pairwise sums and
numpy.linalg.solve.  Only the renders come from the project (metrics.render_depth on the host, tested on its own).

The restatement, the scenes and the helpers take the image ``size`` (default raster_common.SIZE, the camera is
raster_common.camera(size)); a scene dict carries its ``size`` and ``K``, which ``equations`` and ``refine`` pass on."""
import functools

import numpy as np

import raster_common as rc
from betapose_amd import metrics

H, W, K = rc.H, rc.W, rc.K
OK, TOO_FEW, SINGULAR, DIVERGED, REJECTED, NO_IMAGE = 0, 1, 2, 3, 4, 5
ACC = 29
# perturbations of the start poses (see test_icp_host.test_refinement_halves_add) and the refinement's parameters scaled
# to the unit-size meshes: LineMod's 0.02 m is a fifth of its smallest diameter
ROT_DEG, TRANS_FRACT = 3.0, 0.03
MAX_DIST_FRACT = 0.2
P_SCENE = 4

# Host twin against numpy, every entry of the refined poses.  Both take the same pixels (asserted through N) and differ
# in the order of the sums (relative 2 N 2^-53 ~ 2e-13 at N ~ 1000) and in the 6x6 solve (numpy's LAPACK against solve6),
# which the condition number of A, below 2e3 on every pose of these scenes, turns into at most ~ 2e3 * 2e-13 = 4e-10 of a
# step; the steps shrink geometrically, so the issue's 1e-9 holds with room (measured: 4e-15).
POSE_TOL = 1e-9
COND_MAX = 2e3                                  # the condition number that derivation assumes (condition_numbers below)


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def pixel_terms(depth, test, pose, max_dist, min_cos, c=0.0, size=rc.SIZE):
    """Everything the definition says about the pixels of one render [H, W] (0 = nothing drawn) and one test depth image
    in pose units (0 = missing): dict of the boolean mask ``take`` [H, W], ``J`` [H, W, 6], ``r`` [H, W], and the two
    threshold quantities ``cos`` and ``dist`` with the mask ``cand`` of the pixels they were decided on."""
    z = np.asarray(depth, dtype=np.float64)
    zt = np.asarray(test, dtype=np.float64)
    (H, W), K = size, rc.camera(size)
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([(xs + c - K[0, 2]) / K[0, 0], (ys + c - K[1, 2]) / K[1, 1], np.ones((H, W))], axis=-1)
    q = z[..., None] * d
    drawn = z > 0
    cand = np.zeros((H, W), bool)
    cand[1:-1, 1:-1] = (drawn[1:-1, 1:-1] & drawn[1:-1, :-2] & drawn[1:-1, 2:] & drawn[:-2, 1:-1] & drawn[2:, 1:-1]
                        & (zt[1:-1, 1:-1] != 0))
    m = np.zeros((H, W, 3))
    m[1:-1, 1:-1] = np.cross(q[1:-1, 2:] - q[1:-1, :-2], q[2:, 1:-1] - q[:-2, 1:-1])
    ln = np.linalg.norm(m, axis=-1)
    cand &= ln > 0
    n = m / np.where(ln > 0, ln, 1.0)[..., None]
    nd = (n * d).sum(-1)
    flip = nd > 0
    n = np.where(flip[..., None], -n, n)
    nd = np.where(flip, -nd, nd)
    cos = -nd / np.linalg.norm(d, axis=-1)
    dist = np.abs(zt - z)
    take = cand & ~(cos < min_cos) & ~(dist > max_dist)
    r = (zt - z) * nd
    qc = q - np.asarray(pose)[:3, 3]
    J = np.concatenate([np.cross(qc, n), n], axis=-1)
    return {"take": take, "J": J, "r": r, "cos": cos, "dist": dist, "cand": cand}


def accumulate_np(depth, test, pose, max_dist, min_cos, c=0.0, size=rc.SIZE):
    """[29] = A's upper triangle row by row, b, N, E of one render against one test image."""
    t = pixel_terms(depth, test, pose, max_dist, min_cos, c, size)
    J, r = t["J"][t["take"]], t["r"][t["take"]]
    out = np.zeros(ACC)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            out[k] = np.sum(J[:, i] * J[:, j])
            k += 1
    for i in range(6):
        out[21 + i] = np.sum(J[:, i] * r)
    out[27] = len(r)
    out[28] = np.sum(r * r)
    return out


def render(pose, v, f, c=0.0, near=0.01, size=rc.SIZE):
    return metrics.render_depth(np.asarray(pose)[None, :3], v, f, rc.camera(size), size, None, c, near)[0][0]


def normal_equations_np(poses, v, f, test_u16, index, depth_scale, max_dist, min_cos, c=0.0, size=rc.SIZE):
    out = np.zeros((len(poses), ACC))
    for p, pose in enumerate(poses):
        if 0 <= index[p] < len(test_u16):
            out[p] = accumulate_np(render(pose, v, f, c, size=size), test_u16[index[p]].astype(np.float64) * depth_scale, pose,
                                   max_dist, min_cos, c, size)
    return out


def unpack(acc):
    """(A [6, 6], b [6], N, E) of one accumulation."""
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = acc[k]
            k += 1
    return A, acc[21:27].copy(), int(acc[27]), float(acc[28])


def refine_np(poses, v, f, test_u16, index, depth_scale, iterations=8, max_dist=0.02, min_cos=0.25, min_pixels=32, c=0.0,
              size=rc.SIZE):
    """(poses_out [P, 3, 4], stats [P, 6]) by the definition."""
    poses = np.asarray(poses, dtype=np.float64)[:, :3, :4]
    out, stats = poses.copy(), np.zeros((len(poses), 6))
    for p in range(len(poses)):
        if not 0 <= index[p] < len(test_u16):
            stats[p, 5] = NO_IMAGE
            continue
        test = test_u16[index[p]].astype(np.float64) * depth_scale
        pose, status, done = poses[p].copy(), OK, 0

        def measure():
            _, _, N, E = unpack(accumulate_np(render(pose, v, f, c, size=size), test, pose, max_dist, min_cos, c, size))
            return N, (np.sqrt(E / N) if N > 0 else 0.0)
        for k in range(iterations):
            A, b, N, E = unpack(accumulate_np(render(pose, v, f, c, size=size), test, pose, max_dist, min_cos, c, size))
            if k == 0:
                stats[p, 0], stats[p, 1] = N, (np.sqrt(E / N) if N > 0 else 0.0)
            if N < min_pixels:
                status = TOO_FEW
                break
            try:
                xi = np.linalg.solve(A, b)
            except np.linalg.LinAlgError:
                status = SINGULAR
                break
            if np.linalg.norm(xi[:3]) > 0.5 or np.linalg.norm(xi[3:]) > 4 * max_dist:
                status = DIVERGED
                break
            pose[:, :3] = rodrigues(xi[:3]) @ pose[:, :3]
            pose[:, 3] += xi[3:]
            done += 1
        if iterations == 0:
            stats[p, 0], stats[p, 1] = measure()
        stats[p, 2], stats[p, 3] = measure()
        if stats[p, 3] > stats[p, 1]:
            pose, status = poses[p].copy(), REJECTED
            stats[p, 2], stats[p, 3] = stats[p, 0], stats[p, 1]
        out[p], stats[p, 4], stats[p, 5] = pose, done, status
    return out, stats


def perturb(pose, rng, d, rot_deg, trans_fract):
    """The pose turned by ``rot_deg`` degrees about a random axis through the object's origin and moved by
    ``trans_fract`` diameters in a random direction."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    shift = rng.normal(size=3)
    shift /= np.linalg.norm(shift)
    out = np.array(pose, dtype=np.float64)[:3, :4].copy()
    out[:, :3] = rodrigues(axis * np.deg2rad(rot_deg)) @ out[:, :3]
    out[:, 3] += shift * d * trans_fract
    return out


BOX_NORMALS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
BOX_MIN_FACE_COS = 0.35


def box_face_cosines(pose):
    """cos of the angle between each cube face's outward normal and the direction from its centre to the camera."""
    R, t = np.asarray(pose)[:3, :3], np.asarray(pose)[:3, 3]
    c = (BOX_NORMALS * 0.5) @ R.T + t
    return -((BOX_NORMALS @ R.T) * c).sum(-1) / np.linalg.norm(c, axis=-1)


def ground_truth(name, size=rc.SIZE):
    """The scene's P_SCENE ground-truth poses: raster_common.poses_for(name), and for the box those of its first 32 that
    show THREE faces at more than BOX_MIN_FACE_COS each.  Point-to-plane residuals constrain a pose only along the
    normals they see: with one or two faces of a cube inside min_cos the translation along the hidden normals (and the
    rotations about them) is left to the depth noise, the normal matrix is near singular, and no projective ICP can be
    asked to approach the ground truth (test_icp_host.test_box_sliding_poses keeps two such poses and checks what does
    hold there)."""
    if name != "box":
        return rc.poses_for(name, P_SCENE, size)
    cand = rc.poses_for("box", 32, size)
    keep = [p for p in cand if (box_face_cosines(p) > BOX_MIN_FACE_COS).sum() == 3]
    assert len(keep) >= P_SCENE
    return np.stack(keep[:P_SCENE])


def box_sliding_ground_truth():
    """The first two of raster_common.poses_for('box', 32) that show fewer than three faces inside min_cos."""
    cand = rc.poses_for("box", 32)
    keep = [p for p in cand if (box_face_cosines(p) > 0.25).sum() < 3]
    return np.stack(keep[:2])


@functools.lru_cache(maxsize=None)
def scene(name, rot_deg=ROT_DEG, trans_fract=TRANS_FRACT, sliding=False, size=rc.SIZE):
    """dict of one mesh's refinement scene: ground truth = ground_truth(name) (``sliding``: box_sliding_ground_truth);
    test image p is the host render at ground truth p, quantised to uint16 with a quantum of 5e-5 diameters (every depth
    of the pose range stays under 65 535 counts); start pose p is ground truth p perturbed.  ``size`` is the image's and
    fixes the camera (raster_common.camera); the dict carries both.  Computed once per session, read-only."""
    v, f = rc.MESHES[name]()
    d = rc.diameter(v)
    gt = box_sliding_ground_truth() if sliding else ground_truth(name, size)
    depth_scale = 5e-5 * d
    depth = metrics.render_depth(gt, v, f, rc.camera(size), size)[0].astype(np.float64)
    counts = np.round(depth / depth_scale)
    assert counts.max() < 65535
    test = counts.astype(np.uint16)
    rng = np.random.default_rng(rc.SEEDS[name] + 100)
    start = np.stack([perturb(gt[p], rng, d, rot_deg, trans_fract) for p in range(len(gt))])
    index = np.arange(len(gt), dtype=np.int32)
    for a in (v, f, gt, test, start, index):
        a.setflags(write=False)
    return {"v": v, "f": f, "d": d, "gt": gt, "start": start, "test": test, "index": index, "depth_scale": depth_scale,
            "max_dist": MAX_DIST_FRACT * d, "min_cos": 0.25, "size": tuple(size), "K": rc.camera(size)}


@functools.lru_cache(maxsize=None)
def refined_np(name, size=rc.SIZE):
    """refine_np of a scene with the default iterations and min_pixels, once per session."""
    s = scene(name, size=size)
    out, stats = refine_np(s["start"], s["v"], s["f"], s["test"], s["index"], s["depth_scale"], max_dist=s["max_dist"],
                           min_cos=s["min_cos"], size=size)
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


@functools.lru_cache(maxsize=None)
def refined_host(name, size=rc.SIZE):
    s = scene(name, size=size)
    out, stats = metrics.refine_poses_depth(s["start"], s["v"], s["f"], s["K"], s["test"], s["index"], s["depth_scale"],
                                            max_dist=s["max_dist"], min_cos=s["min_cos"])
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


def add(pose_a, pose_b, v):
    return float(metrics.add_err(np.vstack([pose_a[:3], [0, 0, 0, 1]]), np.vstack([pose_b[:3], [0, 0, 0, 1]]), v))


def threshold_margin(poses, s, c=0.0):
    """The smallest distance of any decided pixel of these poses' first accumulation from the max_dist and the min_cos
    threshold: the tests' precondition is that it exceeds 1e-9, so no decision hangs on the last bits."""
    worst = np.inf
    for p, pose in enumerate(poses):
        t = pixel_terms(render(pose, s["v"], s["f"], c, size=s["size"]),
                        s["test"][s["index"][p]].astype(np.float64) * s["depth_scale"], pose, s["max_dist"], s["min_cos"], c,
                        s["size"])
        if t["cand"].any():
            worst = min(worst, np.abs(t["cos"][t["cand"]] - s["min_cos"]).min(),
                        np.abs(t["dist"][t["cand"]] - s["max_dist"]).min())
    return worst


def condition_numbers(acc):
    """The 2-norm condition number of A of every row of normal equations [P, 29]."""
    return np.array([np.linalg.cond(unpack(a)[0]) for a in acc])


def many_scene():
    """raster_common.MANY_CYCLE poses of the box on the MANY_SIZE image, each with the render of its own ground truth as
    test image and a perturbed start: the scene the many-poses test cycles through."""
    size = rc.MANY_SIZE
    v, f = rc.box()
    d = rc.diameter(v)
    gt = rc.many_poses()
    depth_scale = 5e-5 * d
    test = np.round(metrics.render_depth(gt, v, f, rc.camera(size), size)[0].astype(np.float64) / depth_scale).astype(np.uint16)
    rng = np.random.default_rng(141)
    start = np.stack([perturb(gt[p], rng, d, ROT_DEG, TRANS_FRACT) for p in range(len(gt))])
    return {"v": v, "f": f, "d": d, "gt": gt, "start": start, "test": test, "index": np.arange(len(gt), dtype=np.int32),
            "depth_scale": depth_scale, "max_dist": MAX_DIST_FRACT * d, "min_cos": 0.25, "size": size, "K": rc.camera(size)}


def closeup_scene(size):
    """The frame-filling cube of raster_common.edge_cases as an accumulation scene: the test image is the render at that
    pose, the two start poses are it perturbed.  The random-pose scenes keep their objects round the middle of the
    image, so their accepted pixels end before the last rows; here they lie in every row but the border's, and so in
    every 2 048-pixel slice of the device's accumulation, the ragged last one included (take_per_slice shows it)."""
    v, f, gt, _ = rc.edge_cases(size)["box_closeup"]
    d = rc.diameter(v)
    depth_scale = 5e-5 * d
    counts = np.round(metrics.render_depth(gt[None], v, f, rc.camera(size), size)[0].astype(np.float64) / depth_scale)
    assert counts.max() < 65535
    rng = np.random.default_rng(151)
    start = np.stack([perturb(gt, rng, d, ROT_DEG, TRANS_FRACT) for _ in range(2)])
    return {"v": v, "f": f, "d": d, "gt": np.stack([gt, gt]), "start": start, "test": counts.astype(np.uint16),
            "index": np.zeros(2, np.int32), "depth_scale": depth_scale, "max_dist": MAX_DIST_FRACT * d, "min_cos": 0.25,
            "size": tuple(size), "K": rc.camera(size)}


def take_per_slice(pose, p, s, c=0.0, pixels=2048):
    """The numpy restatement's count of accepted pixels of pose ``p`` of scene ``s``, by slice of ``pixels`` flat
    pixel indices (icp.hip ICP_PIX: one block of icp_accumulate_kernel each)."""
    take = pixel_terms(render(pose, s["v"], s["f"], c, size=s["size"]), s["test"][s["index"][p]].astype(np.float64) * s["depth_scale"],
                       pose, s["max_dist"], s["min_cos"], c, s["size"])["take"].reshape(-1)
    return np.add.reduceat(take.astype(np.int64), np.arange(0, take.size, pixels))


def entry_bounds(acc):
    """The issue's bound on every entry of one accumulation: 2 N 2^-53 scale, scale = sqrt(A_ii A_jj) for A_ij,
    sqrt(A_ii E) for b_i (and for E itself sqrt(E E)); the worst case of an f64 sum of N terms."""
    A, _, N, E = unpack(acc)
    u = 2.0 * N * 2.0 ** -53
    out = np.zeros(ACC)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            out[k] = u * np.sqrt(A[i, i] * A[j, j])
            k += 1
    for i in range(6):
        out[21 + i] = u * np.sqrt(A[i, i] * E)
    out[28] = u * E
    return out


def worst_bound_ratio(got, want):
    """The largest |got - want| / entry_bounds(want) over every entry with a bound: what the tests print before
    assert_equations_close asks for <= 1."""
    worst = 0.0
    for g, w in zip(np.asarray(got), np.asarray(want)):
        bound = entry_bounds(w)
        on = bound > 0
        if on.any():
            worst = max(worst, float((np.abs(g - w)[on] / bound[on]).max()))
    return worst


def assert_equations_close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    for p in range(len(want)):
        assert got[p, 27] == want[p, 27], (p, got[p, 27], want[p, 27])
        bound = entry_bounds(want[p])
        diff = np.abs(got[p] - want[p])
        assert np.all(diff <= bound), (p, np.argmax(diff - bound), diff.max())


# ---------------------------------------------------------------- what both test files call and the guard scenes

def equations(s, poses, device=None, **kw):
    return metrics.icp_normal_equations(poses, s["v"], s["f"], s["K"], s["test"], s["index"], s["depth_scale"], s["max_dist"],
                                        s["min_cos"], device=device, **kw)


def refine(s, poses, test=None, index=None, device=None, **kw):
    return metrics.refine_poses_depth(poses, s["v"], s["f"], s["K"], s["test"] if test is None else test,
                                      s["index"] if index is None else index, s["depth_scale"], max_dist=s["max_dist"],
                                      min_cos=s["min_cos"], device=device, **kw)


def guard_cases(s):
    """name -> (test images, index, expected status): situations in which the pose must come back bit for bit."""
    far = np.array(s["gt"])
    far[:, 2, 3] += s["d"]                     # one diameter deeper: every |z_t - z_r| exceeds max_dist = 0.2 diameters
    far_depth = metrics.render_depth(far, s["v"], s["f"], s["K"], s["size"])[0].astype(np.float64)
    far_test = np.round(far_depth / s["depth_scale"]).astype(np.uint16)
    return {"all_zero": (np.zeros_like(s["test"]), s["index"], TOO_FEW),
            "no_image": (s["test"], np.full(len(s["index"]), -1, np.int32), NO_IMAGE),
            "index_T": (s["test"], np.full(len(s["index"]), len(s["test"]), np.int32), NO_IMAGE),
            "far": (far_test, s["index"], TOO_FEW)}


def diverged_scene():
    """The box scene with max_dist = 0.012 diameters: only the pixels that happen to lie within it take part, their normal
    equations no longer describe the pose error, and pose 1's first solution is a translation beyond 4 max_dist (pose 2 has
    too few pixels, poses 0 and 3 still converge)."""
    s = scene("box")
    return dict(s, max_dist=0.012 * s["d"])


def singular_scene():
    """A cube seen face on: every normal is the same, A has rank 3 and the solve finds no pivot (or, should the order of
    the sums leave a pivot of a few ulps, a solution far beyond the step guard)."""
    s = scene("box")
    gt = np.hstack([np.eye(3), [[0.05], [0.03], [3.5]]])[None]
    depth = metrics.render_depth(gt, s["v"], s["f"], K, (H, W))[0].astype(np.float64)
    start = gt.copy()
    start[0, 2, 3] += 0.02
    return dict(s, gt=gt, start=start, test=np.round(depth / s["depth_scale"]).astype(np.uint16), index=np.zeros(1, np.int32))
