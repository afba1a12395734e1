"""Stacks, scenes and restatements shared by test_synth_multi_host.py and test_gpu_synth_multi.py.

``random_stack(size, J)`` is three scenes of ``J`` random depth images whose values come from a handful of numbers, so
exact ties are common; object ``J - 1`` covers no pixel, object 0 is absent from scene 1, every object is absent from
scene 2.  ``rendered_stack(size)`` is real renders: an icosphere, a torus, a box and the SAME icosphere at the SAME
pose again (objects 0 and 3 tie on every pixel they share).  ``numpy_instances`` restates the contract in numpy.  All of
it is computed once per session and read-only."""
import functools
import hashlib
import os

import numpy as np

import raster_common as rc
import synth_common as sc

SIZES = [(48, 64), (75, 113)]          # 113: H W is no multiple of 4 and odd planes are misaligned -- the scalar path
OBJECTS = [1, 3, 32]
IMAGES = 3


def numpy_instances(alone, present):
    """(ids, depth, stats) of the contract, from masks: the masked arg-min with the highest j among equal depths."""
    alone, present = np.asarray(alone), np.asarray(present) != 0
    J, I, H, W = alone.shape
    drawn = (alone > 0) & present.T[:, :, None, None]
    key = np.where(drawn, alone, np.float32(np.inf))
    best = key.min(axis=0)
    winners = drawn & (key == best[None])
    some = winners.any(axis=0)
    top = J - 1 - np.argmax(winners[::-1], axis=0)
    ids = np.where(some, top + 1, 0).astype(np.uint8)
    depth = np.where(some, best, np.float32(0)).astype(np.float32)

    def box(mask):
        ys, xs = np.nonzero(mask)
        return [xs.min(), xs.max(), ys.min(), ys.max()] if len(xs) else [-1] * 4
    stats = np.zeros((I, J, 10), np.int32)
    for i in range(I):
        for j in range(J):
            full, vis = alone[j, i] > 0, ids[i] == j + 1
            stats[i, j] = [full.sum(), vis.sum()] + box(full) + box(vis)
    return ids, depth, stats


@functools.lru_cache(maxsize=None)
def random_stack(size, J, images=IMAGES, seed=0):
    """(alone [J, I, H, W] float32, present [I, J] uint8)."""
    H, W = size
    rng = np.random.default_rng([20261021, H, W, J, seed])
    levels = np.array([0, 0, 0.5, 0.75, 1.0, 1.25, 1.5], np.float32)            # two of seven are background
    alone = levels[rng.integers(0, len(levels), (J, images, H, W))]
    alone[J - 1] = 0                                                             # covers no pixel
    present = np.ones((images, J), np.uint8)
    if images > 1:
        present[1, 0] = 0
    if images > 2:
        present[2] = 0
    alone.setflags(write=False)
    present.setflags(write=False)
    return alone, present


@functools.lru_cache(maxsize=None)
def host_instances(size, J):
    from betapose_amd import synth
    out = synth.instance_masks(*random_stack(size, J))
    for a in out:
        a.setflags(write=False)
    return out


def render_objects():
    """[(vertices, faces, colours BGR)] of rendered_stack, in metres; object 3 IS object 0."""
    sv, sf = rc.icosphere()
    tv, tf = rc.torus()
    bv, bf = rc.box()
    ico = (sv * 0.05, sf, sc.vertex_colors(len(sv), 21))
    return [ico, (tv * 0.03, tf, sc.vertex_colors(len(tv), 22)), (bv * 0.07, bf, sc.vertex_colors(len(bv), 23)),
            (ico[0], ico[1], sc.vertex_colors(len(sv), 24))]


@functools.lru_cache(maxsize=None)
def rendered_stack(size):
    """(alone [4, 3, H, W], poses [3, 4, 3, 4], present [3, 4]): three scenes with the objects near the optical axis at
    staggered depths, so they overlap; scene 1 lacks the box, scene 2 lacks object 3 (so object 0 shows there)."""
    from betapose_amd import metrics
    H, W = size
    K = rc.camera(size)
    rng = np.random.default_rng(31)
    objs = render_objects()
    poses = np.zeros((3, 4, 3, 4))
    order = [[0, 1, 2], [2, 0, 1], [0, 2, 1]]               # nearest first: object 0 is in front where object 3 is absent
    for i in range(3):
        for j in range(3):
            poses[i, j, :, :3] = rc.rand_rot(rng)
            poses[i, j, :, 3] = [rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02), 0.25 + 0.05 * order[i][j] + rng.uniform(0, 0.02)]
        poses[i, 3] = poses[i, 0]
    alone = np.stack([metrics.render_depth(poses[:, j], objs[j][0], objs[j][1], K, size)[0] for j in range(4)])
    present = np.ones((3, 4), np.uint8)
    present[1, 2] = 0
    present[2, 3] = 0
    assert (alone.reshape(4, 3, -1) > 0).any(axis=2).all() and np.array_equal(alone[0], alone[3])
    for a in (alone, poses, present):
        a.setflags(write=False)
    return alone, poses, present


# ---- synthesize_multi's own scenes: four small meshes, millimetres as a tree stores them
MULTI_SIZE = (48, 64)
MULTI_IDS = [1, 5, 6, 9]
MULTI_MIN_VISIB = 0.3
# chosen on the CPU: the first seed from 0 whose four scenes hold all three kinds test_synth_multi_host.py asserts.  It
# drops three objects (object 6 from scene 1, objects 1 and 5 from scene 3); the survivors' visib_fract are
# 0.58 0.33 0.47 1.00 / 0.86 0.75 - 0.99 / 0.89 0.35 0.70 0.63 / - - 0.84 1.00: eleven partly hidden, two whole.
MULTI_SEED = 0


def multi_meshes():
    sv, sf = rc.icosphere()
    tv, tf = rc.torus()
    bv, bf = rc.box()
    return {1: (sv * 50.0, sf, sc.vertex_colors(len(sv), 11)), 5: (tv * 30.0, tf, sc.vertex_colors(len(tv), 12)),
            6: (bv * 70.0, bf, sc.vertex_colors(len(bv), 13)), 9: (sv * 35.0, sf, sc.vertex_colors(len(sv), 14))}


def multi_meshes_metres():
    m = multi_meshes()
    return [(m[o][0] * 0.001, m[o][1], m[o][2]) for o in MULTI_IDS]


def synthesize_multi(n=4, device=None, first_scene=0, seed=None, min_visib=MULTI_MIN_VISIB):
    from betapose_amd import synth
    return synth.synthesize_multi(multi_meshes_metres(), rc.camera(MULTI_SIZE), MULTI_SIZE, n, MULTI_SEED if seed is None else seed,
                                  obj_ids=MULTI_IDS, min_visib=min_visib, sensor=dict(noise_k=0, hole_p=0),
                                  first_scene=first_scene, device=device)


@functools.lru_cache(maxsize=None)
def host_multi():
    out = synthesize_multi(4)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- trees
def tree_digest(base):
    """SHA-256 over a tree's relative paths and files in sorted order: a PNG counts as its decoded pixels (shape, type and
    bytes: the compressed stream is the zlib build's business), every other file as its bytes."""
    from PIL import Image
    h = hashlib.sha256()
    for dirpath, dirs, names in os.walk(base):
        dirs.sort()
        for n in sorted(names):
            path = os.path.join(dirpath, n)
            with open(path, "rb") as f:
                data = f.read()
            if n.endswith(".png"):
                a = np.asarray(Image.open(path))
                data = str((a.shape, a.dtype.str)).encode() + np.ascontiguousarray(a).tobytes()
            h.update(os.path.relpath(path, base).replace(os.sep, "/").encode() + b"\0" + data + b"\0")
    return h.hexdigest()


# tree_digest of what the commit BEFORE synthesize_multi wrote, recorded there: write_scene_tree of synth_common's four
# scenes, and synthesize.py --model with test_synth_host.py's command line.  Scenes of one target must keep them.
SINGLE_TREE_DIGEST = "f72997b844903ba04419f46232fc834d1d6c7e3b4ed010f57132ea9426f3ee22"
SINGLE_CLI_DIGEST = "d9f666cb5d836099ec43ecf3674ed96b32c75e13aaa16c3811ac467cb1b68377"
SINGLE_CLI_ARGS = ["--obj_id", "1", "--frames", "3", "--size", "48x64", "--camera", "60,60,31.5,23.5", "--seed", "3"]
