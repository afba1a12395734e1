"""Scenes, parameter tables and sizes shared by test_synth_host.py and test_gpu_synth.py.

``scene_stack(size)`` is five renders on the host, computed once per session and read-only:
  0  an icosphere whose centre projects to pixel (0, 0): cut by the left and the top border;
  1  a torus whose centre projects to (W - 1, H - 1): cut by the right and the bottom border;
  2  nothing: no foreground;
  3  a rectangle past every border: the foreground fills the image;
  4  a torus round the middle, which hides part of itself and has a hole (background inside the silhouette).
The backgrounds are seeded random bytes, so nothing of the code under test makes its own input.  ``COMPOSE_CASES`` are
the six (radius, feather) pairs, each with five different rows of gains, offsets and sigmas; ``SENSOR_ROWS`` the five
sensor rows (no noise and no holes; typical; strong noise with every edge a hole; holes only; extreme noise)."""
import functools

import numpy as np

import raster_common as rc

SIZES = [(48, 64), (75, 113)]
TALL = (129, 67)
SEED = 20261021
DEPTH_SCALE = 0.001
COMPOSE_CASES = [(r, feather) for r in (0, 1, 2) for feather in (0, 1)]
SENSOR_ROWS = np.array([[0, 0, 0], [512, 30, 128], [2000, 5, 256], [0, 10, 256], [65535, 0, 77]], np.int32)
IMAGES = 5


def vertex_colors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene_stack(size):
    """(color [5, H, W, 3] uint8, depth [5, H, W] float32) as the docstring lists them."""
    from betapose_amd import metrics
    (H, W), K = size, rc.camera(size)
    sv, sf = rc.icosphere()
    tv, tf = rc.torus()
    rot = rc.rand_rot(np.random.default_rng(5))
    at = lambda u, v, z: [(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z]
    color = np.zeros((IMAGES, H, W, 3), np.uint8)
    depth = np.zeros((IMAGES, H, W), np.float32)
    one = lambda i: np.array([i], np.int32)

    def draw(i, v, f, pose, seed):
        nonlocal color, depth
        color, depth, _ = metrics.render_color(np.asarray(pose)[None], v, f, vertex_colors(len(v), seed), K, size,
                                               image_index=one(i), images=IMAGES, into=(color, depth))
    draw(0, sv, sf, np.hstack([rot, np.array(at(0, 0, 3.0))[:, None]]), 1)
    draw(1, tv, tf, np.hstack([rot, np.array(at(W - 1, H - 1, 3.5))[:, None]]), 2)
    rv, rf = rc.pixel_rect(-5, -5, W + 5, H + 5, 2.0, size)
    draw(3, rv, rf, np.eye(4)[:3], 3)
    draw(4, tv, tf, rc.poses_for("torus", 1, size)[0], 4)
    assert depth[0, 0, :].any() and depth[0, :, 0].any() and depth[1, -1, :].any() and depth[1, :, -1].any()
    assert not depth[2].any() and (depth[3] > 0).all()
    assert 0 < (depth[4] > 0).mean() < 1
    color.setflags(write=False)
    depth.setflags(write=False)
    return color, depth


@functools.lru_cache(maxsize=None)
def backgrounds(size, images=IMAGES):
    b = np.random.default_rng(77).integers(0, 256, (images,) + tuple(size) + (3,)).astype(np.uint8)
    b.setflags(write=False)
    return b


def compose_table(r, feather, images=IMAGES):
    """Five different rows of one (radius, feather) pair: row 0 is the neutral camera, the others draw their gains
    (0.75 .. 1.5), offsets (-40 .. 40) and sigmas (0 .. 12 grey levels) from a seeded generator."""
    rng = np.random.default_rng(100 + 10 * r + feather)
    rows = [[feather, r, 256, 256, 256, 0, 0, 0, 0]]
    for _ in range(images - 1):
        rows.append([feather, r] + rng.integers(192, 385, 3).tolist() + rng.integers(-40, 41, 3).tolist() + [int(rng.integers(0, 3073))])
    return np.array(rows, np.int32)


@functools.lru_cache(maxsize=None)
def host_compose(size, r, feather):
    from betapose_amd import synth
    color, depth = scene_stack(size)
    out = synth.compose(backgrounds(size), color, depth, compose_table(r, feather), SEED, 7)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_sensor(size):
    from betapose_amd import synth
    out = synth.sensor_depth(scene_stack(size)[1], DEPTH_SCALE, SENSOR_ROWS, SEED, 7)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_background(size):
    from betapose_amd import synth
    out = synth.procedural_background(3, size, SEED, 7)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bank():
    b = np.random.default_rng(78).integers(0, 256, (2, 37, 53, 3)).astype(np.uint8)
    b.setflags(write=False)
    return b


# bank image, x0, y0, w, h, flip: the whole photograph, a window enlarged, one reduced to a single column, one flipped
WINDOWS = np.array([[0, 0, 0, 53, 37, 0], [1, 5, 3, 20, 11, 0], [0, 52, 0, 1, 37, 0], [1, 10, 10, 43, 27, 1]], np.int32)


@functools.lru_cache(maxsize=None)
def host_windows(size):
    from betapose_amd import synth
    out = synth.background_windows(bank(), WINDOWS, size)
    out.setflags(write=False)
    return out


# ---- the synthesiser's own scenes: a 10 cm icosphere target and a torus occluder, in millimetres as a tree stores them
SCENES_SIZE = (48, 64)
SCENES_SEED = 3          # chosen on the CPU: its four scenes have visib_fract 0.81, 0.80, 0.61, 0.50 (test_synth_host.py checks 0 < . < 1)


def scene_meshes():
    sv, sf = rc.icosphere()
    tv, tf = rc.torus()
    return {1: (sv * 50.0, sf, vertex_colors(len(sv), 11)), 2: (tv * 30.0, tf, vertex_colors(len(tv), 12))}


def synthesize(n=4, device=None, first_scene=0, sensor=None, seed=SCENES_SEED, size=SCENES_SIZE):
    from betapose_amd import synth
    m = scene_meshes()
    metres = lambda mesh: (mesh[0] * 0.001, mesh[1], mesh[2])
    return synth.synthesize_scenes(metres(m[1]), [metres(m[2])], rc.camera(size), size, n, seed,
                                   sensor=dict(noise_k=0, hole_p=0) if sensor is None else sensor, first_scene=first_scene,
                                   device=device)
