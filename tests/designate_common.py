"""Case builders shared by test_designate_host.py and test_gpu_designate.py: the three-bump scene whose key points are
known, its octave clouds, clouds with duplicated points, and the numpy restatements of DESIGN.md 3.9."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUMPS = ((10.0, 10.0, 4.0, 2.5), (28.0, 14.0, -3.0, 3.0), (18.0, 30.0, 5.0, 2.0))      # (cx, cy, height, sigma)
SCENE_ARGS = dict(min_scale=1.0, n_octaves=3, n_scales_per_octave=3)
OCTAVE_SIZES = [1215, 490, 154]


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene():
    """41 x 41 jittered grid points on a surface of three Gaussian bumps, [1681, 3] float64 (read-only)."""
    rng = np.random.default_rng(3)
    x, y = np.meshgrid(np.arange(41.0), np.arange(41.0), indexing="ij")
    x, y = x.ravel(), y.ravel()
    x = x + rng.uniform(-0.2, 0.2, 1681)
    y = y + rng.uniform(-0.2, 0.2, 1681)
    z = np.zeros_like(x)
    for cx, cy, h, s in BUMPS:
        z = z + h * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    return _frozen(np.stack([x, y, z], axis=1))


@functools.lru_cache(maxsize=None)
def octave_clouds():
    """The scene's cloud and scales of each of its three octaves: [(cloud, scales), ...] (read-only)."""
    from betapose_amd import designate as D
    cloud, out = scene(), []
    for o in range(3):
        cloud = D.voxel_grid(cloud, 1.0 * 2.0 ** o)
        out.append((_frozen(cloud), _frozen(D.octave_scales(1.0, o, 3))))
    return out


@functools.lru_cache(maxsize=None)
def with_duplicates(n):
    """n points of the scene's first octave cloud nearest to the first bump, three of them repeated at other places of
    the array (so ties in distance and in value occur), read-only."""
    cloud = octave_clouds()[0][0]
    order = np.argsort(np.hypot(cloud[:, 0] - BUMPS[0][0], cloud[:, 1] - BUMPS[0][1]), kind="stable")
    pts = cloud[np.sort(order[:n])].copy()
    for src, dst in ((3, n - 2), (n // 2, 5), (n - 7, n // 3)):
        pts[dst] = pts[src]
    return _frozen(pts)


@functools.lru_cache(maxsize=None)
def nearest_part(n):
    """The n points of the scene's first octave cloud nearest to the first bump, in cloud order (read-only)."""
    cloud = octave_clouds()[0][0]
    order = np.argsort(np.hypot(cloud[:, 0] - BUMPS[0][0], cloud[:, 1] - BUMPS[0][1]), kind="stable")
    return _frozen(cloud[np.sort(order[:n])])


def pair_d2(p):
    d = p[:, None, :] - p[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dog_oracle(points, field, scales):
    """DoG [n, ns-1] from the definition, with libm's exp and numpy's sums."""
    d2 = pair_d2(points)
    f = points[:, field]
    G = []
    for s in scales:
        w = np.where(d2 <= 9.0 * (s * s), np.exp(-0.5 * d2 / (s * s)), 0.0)
        G.append((w @ f) / w.sum(axis=1))
    G = np.stack(G, axis=1)
    return G[:, 1:] - G[:, :-1]


def flags_oracle(points, dog, k, min_contrast):
    """flags [n, ns-3] recomputed from a DoG array: pure comparisons, hence exact."""
    n, nd = dog.shape
    d2 = pair_d2(points)
    kk = min(k, n)
    flags = np.zeros((n, nd - 2), np.int8)
    idx = np.arange(n)
    for p in range(n):
        nb = np.lexsort((idx, d2[p]))[:kk]          # by (d2, index)
        for j in range(1, nd - 1):
            v = dog[p, j]
            if not abs(v) >= min_contrast:
                continue
            block = dog[nb, j - 1:j + 2]
            if v < dog[p, j - 1] and v < dog[p, j + 1] and (v <= block).all():
                flags[p, j - 1] = -1
            elif v > dog[p, j - 1] and v > dog[p, j + 1] and (v >= block).all():
                flags[p, j - 1] = 1
    return flags


def fps_oracle(points, K, start=None):
    """The ten-line loop: (indices, d2)."""
    c = np.zeros(3)
    for row in points:                               # (summed in index order)
        c = c + row
    c = c / len(points)
    from_c = pair_d2(np.vstack([c, points]))[0, 1:]
    idx = [int(np.argmax(from_c)) if start is None else start]
    d2 = [from_c[idx[0]]]
    mind = np.full(len(points), np.inf)
    for _ in range(K - 1):
        d = points - points[idx[-1]]
        mind = np.minimum(mind, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        idx.append(int(np.argmax(mind)))             # (argmax takes the first of equals)
        d2.append(mind[idx[-1]])
    return np.array(idx, np.int32), np.array(d2)


def thin_cloud(n, seed=11, spread=60.0):
    """n random points in a cube of side `spread` with three duplicated points (read-only)."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.0, spread, (n, 3))
    for src, dst in ((2, n - 3), (n // 2, 7), (n - 5, n // 4)):
        pts[dst] = pts[src]
    return _frozen(pts)


def far_cloud(n=10):
    """n points all at least 100 apart: the thinning's pure-quirk case (read-only)."""
    rng = np.random.default_rng(5)
    return _frozen(np.stack([150.0 * np.arange(n), rng.uniform(0, 20, n), rng.uniform(0, 20, n)], axis=1))
