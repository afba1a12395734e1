"""Key-point designation (stage 1 of the reference, ``1_keypoint_designator/main.cpp``): 3-D SIFT key points of a mesh's
vertices, a farthest-point alternative, and the thinning to ``total_kp`` points that ``Model3D.refine`` does.

The wrappers follow annotate.py: ``device=None`` runs the host twin of libbetapose_hip.so (no GPU needed), a torch
device the kernels of csrc/designate.hip; the two agree bit for bit.  Definitions and limits: DESIGN.md 3.9.  The
detector restates PCL's SIFTKeypoint from its published description and has never been compared with PCL's output.
"""
from __future__ import annotations

import os

import numpy as np

MAX_SCALES = 12             # csrc/designate.h DESIGNATE_MAX_SCALES
MAX_K = 64                  # DESIGNATE_MAX_K
MAX_OCTAVE_POINTS = 1 << 17
MAX_FPS_POINTS = 1 << 20
MAX_THIN_POINTS = 1 << 14


def _points(points, name="points"):
    p = np.ascontiguousarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3 or len(p) < 1:
        raise ValueError("%s must be [n, 3] with n >= 1" % name)
    if not np.isfinite(p).all():
        raise ValueError("%s must be finite" % name)
    return p


def voxel_grid(points, leaf):
    """Centroids of the occupied cells of a grid of size ``leaf`` (cell ``floor(p / leaf)`` per axis), in ascending
    cell-key order, each summed in input order.  A grid of more than INT32_MAX cells returns the cloud unchanged
    (PCL's "leaf size is too small").  Host only: both paths of sift_keypoints share it."""
    from . import _lib
    p = _points(points)
    out = np.empty_like(p)
    n_out = _lib.C.c_int(0)
    _lib.check(_lib.lib().bp_voxel_grid_host(_lib.ptr(p), len(p), float(leaf), _lib.ptr(out), _lib.C.byref(n_out)))
    return out[:n_out.value].copy()


def sift_octave(points, field, scales, k=25, min_contrast=0.2, device=None):
    """One octave: ``(dog [n, ns-1] float64, flags [n, ns-3] int8)``.  ``field`` 0 / 1 / 2 takes the x / y / z
    coordinate as the scalar the detector blurs; ``scales`` are the ascending Gaussian sigmas.  ``flags[p, j-1]`` is -1 /
    +1 where ``dog[p, j]`` is a minimum / maximum over the point's three scales and its ``min(k, n)`` nearest points'
    (itself among them) and at least ``min_contrast`` in magnitude."""
    from . import _lib
    p = _points(points)
    sc = np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)
    n, ns = len(p), len(sc)
    if ns < 4:
        raise ValueError("at least 4 scales")
    side = _lib.Side(device)
    dog, flags = side.empty((n, ns - 1), np.float64), side.empty((n, ns - 3), np.int8)
    side.call("bp_sift_octave", side.put(p), n, int(field), _lib.ptr(sc), ns, int(k), float(min_contrast), dog, flags)
    return side.get(dog), side.get(flags)


def octave_scales(min_scale, octave, n_scales_per_octave):
    """``sigma0 * 2^((i - 1) / S)`` for ``i = 0 .. S + 2`` with ``sigma0 = min_scale * 2^octave``."""
    S = int(n_scales_per_octave)
    s0 = float(min_scale) * 2.0 ** int(octave)
    return np.array([s0 * 2.0 ** ((i - 1) / S) for i in range(S + 3)], dtype=np.float64)


def sift_keypoints(points, min_scale=0.01, n_octaves=10, n_scales_per_octave=5, min_contrast=0.2, field=2, k=25,
                   min_points=25, device=None, return_sizes=False):
    """3-D SIFT key points ``[m, 6] = (x, y, z, scale, octave, sign)``; the defaults are the reference's.  Per octave
    ``o`` the cloud is voxel-gridded at ``sigma0 = min_scale * 2^o`` (cumulatively), the detection stops when fewer
    than ``min_points`` points remain, and every non-zero flag gives a row, in (point, scale) order.
    ``return_sizes``: also the list of the octaves' cloud sizes."""
    cloud = _points(points)
    S = int(n_scales_per_octave)
    if S < 1 or S + 3 > MAX_SCALES:
        raise ValueError("n_scales_per_octave must lie in [1, %d]" % (MAX_SCALES - 3))
    if not float(min_scale) > 0:
        raise ValueError("min_scale must be positive")
    rows, sizes = [], []
    for o in range(int(n_octaves)):
        scales = octave_scales(min_scale, o, S)
        cloud = voxel_grid(cloud, float(min_scale) * 2.0 ** o)
        if len(cloud) < int(min_points):
            break
        sizes.append(len(cloud))
        _, flags = sift_octave(cloud, field, scales, k, min_contrast, device)
        pi, ji = np.nonzero(flags)
        for p, j in zip(pi, ji):
            rows.append((cloud[p, 0], cloud[p, 1], cloud[p, 2], scales[j + 1], float(o), float(flags[p, j])))
    kp = np.array(rows, dtype=np.float64).reshape(-1, 6)
    return (kp, sizes) if return_sizes else kp


def farthest_points(points, K, start=None, device=None):
    """Farthest-point sampling: ``(indices [K] int32, d2 [K] float64)``.  ``start`` defaults to the point farthest
    from the centroid; every next index is the point with the largest squared distance to the chosen ones (ties: the
    lowest index), and ``d2`` that distance (for the first: its squared distance from the centroid)."""
    from . import _lib
    p = _points(points)
    n, K = len(p), int(K)
    st = -1 if start is None else int(start)
    if start is not None and not 0 <= st < n:
        raise ValueError("start must lie in [0, n)")
    side = _lib.Side(device)
    idx, d2 = side.empty(max(K, 1), np.int32), side.empty(max(K, 1), np.float64)       # (K < 1 raises in the library)
    side.call("bp_farthest_points", side.put(p), n, K, st, idx, d2)
    return side.get(idx), side.get(d2)


def thin_tail(survivors, rounds_left, position):
    """The rounds of ``Model3D.refine`` after its smallest distance has reached 100.0: each deletes the carried
    ``position`` again, so positions ``position .. position + rounds_left - 1`` of ``survivors`` go; IndexError where
    numpy's ``delete`` raises one."""
    survivors = np.asarray(survivors)
    if rounds_left > 0 and position + rounds_left > len(survivors):
        # (the round that fails is the first one that finds no more than `position` rows left)
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (position, min(position, len(survivors))))
    return np.delete(survivors, np.arange(position, position + max(rounds_left, 0)))


def thin_points(points, keep, device=None):
    """Indices (ascending, int64) of the points ``metrics.refine_keypoints(points, keep)`` keeps, without its
    ``[n, n, 3]`` array per round: every round deletes the first point, in row-major pair order, of the closest pair;
    once the smallest distance is 100.0 or more the reference's two quirks delete a carried position instead
    (thin_tail)."""
    from . import _lib
    p = _points(points)
    n, keep = len(p), int(keep)
    side = _lib.Side(device)
    alive, state = side.empty(n, np.uint8), side.zeros(2, np.int32)
    side.call("bp_thin_points", side.put(p), n, keep, alive, state)
    survivors, state = np.flatnonzero(side.get(alive)), side.get(state)
    return thin_tail(survivors, max(0, n - keep) - int(state[0]), int(state[1]))


def designate(vertices, total_kp=50, method="sift", device=None, return_info=False, **sift_args):
    """Key points ``[m, 3]`` of a mesh's vertices.  ``method='sift'``: sift_keypoints (``sift_args`` are its options),
    thinned to ``total_kp`` by thin_points; when the detector finds no more than ``total_kp`` they are returned as they
    are (object 10 of the reference has 17).  ``method='fps'``: ``total_kp`` farthest points.  ``return_info``: also a
    dict with ``octave_sizes``, ``found`` and ``kept``."""
    v = _points(vertices, "vertices")
    total_kp = int(total_kp)
    if total_kp < 1:
        raise ValueError("total_kp must be positive")
    info = {"octave_sizes": [], "found": 0}
    if method == "sift":
        kp, sizes = sift_keypoints(v, device=device, return_sizes=True, **sift_args)
        info.update(octave_sizes=sizes, found=len(kp))
        out = kp[:, :3]
        if len(out) > total_kp:
            if len(out) > MAX_THIN_POINTS:
                raise ValueError("%d key points found, thin_points takes at most %d: raise min_contrast"
                                 % (len(out), MAX_THIN_POINTS))
            out = out[thin_points(out, total_kp, device)]
    elif method == "fps":
        if sift_args:
            raise ValueError("method 'fps' takes no detector options")
        idx, _ = farthest_points(v, min(total_kp, len(v)), device=device)
        info["found"] = len(idx)
        out = v[idx]
    else:
        raise ValueError("method must be 'sift' or 'fps'")
    out = np.ascontiguousarray(out, dtype=np.float64)
    info["kept"] = len(out)
    return (out, info) if return_info else out


def write_ply(path, points):
    """Key points as an ASCII .ply in the layout of the reference's ``assets/sifts/*.ply``: float x, y, z, one vertex
    per line with a trailing blank, the values rounded to float32 and printed with 12 significant digits."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3).astype(np.float32)
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "end_header\n" % len(p))
        for row in p:
            f.write("%.12g %.12g %.12g \n" % (float(row[0]), float(row[1]), float(row[2])))
