"""Images, numpy restatements and scenes shared by test_verify_host.py and test_gpu_verify.py (pose verification by
gradient agreement).

``SIZES`` and what each opens in csrc/verify.hip (tiles of 64 x 16 pixels, a lane owns four pixels of a row):
  (3, 3)     the smallest image reflect-101 admits: every fetched pixel but the centre's comes through the border.
  (3, 8)     shorter than a tile and two lanes wide.
  (5, 7)     narrower and shorter than one tile, W not a multiple of 4 (the scalar loads and stores).
  (37, 53)   three tile rows, the last of 5 pixel rows; one partial tile column; 3 W = 159 (byte loads).
  (48, 64)   exactly 3 x 1 tiles; 3 W = 192 is a multiple of 16: the staged 16-byte loads, 16-byte stores.
  (20, 80)   3 W = 240: the staged path with TWO tile columns, the second partial (16 of 64 pixels), so words past the
             row's end are skipped and the right border is reflected inside a staged tile; two tile rows, 4 px in the last.
  (70, 130)  5 x 3 tiles, partial in both directions (6 rows, 2 columns); 3 W = 390 (byte loads), W % 4 != 0.
"""
import functools

import numpy as np

import raster_common as rc

SIZES = [(3, 3), (3, 8), (5, 7), (37, 53), (48, 64), (20, 80), (70, 130)]
SCENE_MIN_SQ = 25
RENDER_MIN_SQ = 1624975
D = np.array([-1, -2, 0, 2, 1], np.int64)
S = np.array([1, 4, 6, 4, 1], np.int64)


@functools.lru_cache(maxsize=None)
def images(size):
    """The test images of one size: (names, stack [N, H, W, 3] uint8).  A constant image (everything masked), random
    bytes, random values in 0 .. 3 (many pixels at m2 around 25: the integer mask), and a bright line on each of the four
    border rows and columns (reflect-101)."""
    H, W = size
    rng = np.random.default_rng(1000 * H + W)
    out = {"constant": np.full((H, W, 3), 97, np.uint8),
           "random": rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
           "low": rng.integers(0, 4, (H, W, 3), dtype=np.uint8)}
    for name, sl in (("top", (0, slice(None))), ("bottom", (H - 1, slice(None))), ("left", (slice(None), 0)),
                     ("right", (slice(None), W - 1))):
        im = np.full((H, W, 3), 10, np.uint8)
        im[sl] = (250, 200, 90)
        out["line_" + name] = im
    names = tuple(out)
    stack = np.stack([out[n] for n in names])
    stack.setflags(write=False)
    return names, stack


def gray_ref(img, red):
    a = img.astype(np.int64)
    return (4899 * a[..., red] + 9617 * a[..., 1] + 1868 * a[..., 2 - red] + 8192) >> 14


def sobel_ref(img, red):
    """Integer (gx, gy) [H, W] of one image: np.pad(mode="reflect") is reflect-101, then integer correlation."""
    g = np.pad(gray_ref(img, red), 2, mode="reflect")
    H, W = img.shape[:2]
    gx, gy = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for i in range(5):
        for j in range(5):
            win = g[i:i + H, j:j + W]
            gx += S[i] * D[j] * win
            gy += D[i] * S[j] * win
    return gx, gy


@functools.lru_cache(maxsize=None)
def gradients_ref(size, red, min_sq):
    """Per image of ``images(size)``: integer gx, gy [N, H, W], the kept mask, and float64 unit vectors [N, H, W, 2]."""
    _, stack = images(size)
    gx, gy = map(np.stack, zip(*(sobel_ref(im, red) for im in stack)))
    m2 = gx * gx + gy * gy
    kept = m2 >= min_sq
    mag = np.sqrt(m2.astype(np.float64)) + 0.001
    unit = np.where(kept[..., None], np.stack([gx, gy], -1) / mag[..., None], 0.0)
    for a in (gx, gy, kept, unit):
        a.setflags(write=False)
    return gx, gy, kept, unit


def units_f32_ref(gx, gy, kept):
    """The definition's own float32 steps in numpy (whose float32 square root and quotient are correctly rounded):
    mag = sqrt(float32(m2)) + float32(0.001), n = float32(g) / mag; zeros where masked."""
    m2 = (gx * gx + gy * gy).astype(np.float32)
    mag = np.sqrt(m2) + np.float32(0.001)
    assert mag.dtype == np.float32
    g = np.stack([gx, gy], -1).astype(np.float32)
    return np.where(kept[..., None], g / np.where(kept, mag, np.float32(1))[..., None], np.float32(0)).astype(np.float32)


def score_case(size):
    """Renders, frames and frame indices of one size: every image as a render, two of them as frames, several renders
    per frame in a non-monotonic order."""
    _, stack = images(size)
    frames = np.ascontiguousarray(stack[[1, 2]])                       # random, low
    index = np.array([1, 0, 1, 1, 0, 0, 1], np.int32)[:len(stack)]
    return stack, frames, index


def scores_ref(size, red, render_min_sq, scene_min_sq=SCENE_MIN_SQ):
    """float64 restatement with an unquantised sum: (scores [P], counts [P]) of score_case(size)."""
    stack, frames, index = score_case(size)
    _, _, rkept, runit = gradients_ref(size, red, render_min_sq)
    _, _, _, sunit_all = gradients_ref(size, red, scene_min_sq)
    sunit = sunit_all[[1, 2]]
    scores, counts = np.zeros(len(stack)), np.zeros(len(stack), np.int64)
    for p in range(len(stack)):
        t = np.abs((runit[p] * sunit[index[p]]).sum(-1))[rkept[p]]
        counts[p] = int(rkept[p].sum())
        scores[p] = t.sum() / (counts[p] + 1)
    return scores, counts


def bits(a):
    """An array's bytes as unsigned integers of its item size: NaN rows compare equal when their bits are."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- discrimination: a vertex-coloured mesh at a seeded true pose over a random-texture background
DISC_SIZES = [(48, 64), (70, 130)]
DISC_SEEDS = [0, 1, 2, 3]                                  # x 2 sizes = 8 cases
ROT_DEG = (10.0, 20.0, 45.0, 90.0)                         # perturbation rotations about seeded axes
SHIFT_FRACTION = (0.10, 0.25)                              # ... and translations, fractions of the diameter


@functools.lru_cache(maxsize=None)
def colored_mesh():
    v, f = rc.torus()
    colors = np.random.default_rng(77).integers(0, 256, (len(v), 3), dtype=np.uint8)
    return v, f, colors


def axis_angle(axis, deg):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def pose_pool(seed, size):
    """[1 + 4 + 4, 3, 4]: the true pose, then rotations of ROT_DEG about seeded axes (about the object's centre) and
    in-image-plane translations of SHIFT_FRACTION of the diameter along seeded directions and their opposites."""
    v, _, _ = colored_mesh()
    d = rc.diameter(v)
    rng = np.random.default_rng(500 + seed)
    true = np.zeros((3, 4))
    true[:, :3] = rc.rand_rot(rng)
    z = d * rng.uniform(1.4, 1.7)
    true[:, 3] = [rng.uniform(-3, 3) * z / 60.0, rng.uniform(-2, 2) * z / 60.0, z]
    pool = [true]
    for deg in ROT_DEG:
        p = true.copy()
        p[:, :3] = axis_angle(rng.normal(size=3), deg) @ true[:, :3]
        pool.append(p)
    for frac in SHIFT_FRACTION:
        a = rng.uniform(0, 2 * np.pi)
        for sgn in (1.0, -1.0):
            p = true.copy()
            p[:, 3] += sgn * frac * d * np.array([np.cos(a), np.sin(a), 0.0])
            pool.append(p)
    return np.stack(pool)


def disc_scene(seed, size, device=None):
    """(poses [9, 3, 4], frame [1, H, W, 3] uint8): the mesh rendered at pool[0] pasted over a random-texture background."""
    from betapose_amd import metrics
    v, f, colors = colored_mesh()
    pool = pose_pool(seed, size)
    H, W = size
    rng = np.random.default_rng(900 + seed)
    coarse = rng.integers(0, 256, ((H + 3) // 4, (W + 3) // 4, 3), dtype=np.uint8)
    bg = np.kron(coarse, np.ones((4, 4, 1), np.uint8))[:H, :W]          # 4 x 4 px blocks of random colour
    color, depth, _ = metrics.render_color(pool[:1], v, f, colors, rc.camera(size), size, device)
    frame = metrics.overlay(bg[None], color, depth, 256, device)
    return pool, frame
