"""The training-scene synthesiser on the host twins (no GPU): every kernel's twin against a numpy restatement written here
from DESIGN.md 3.15's text, the identities, the noise statistics, the sensor model, chunking, the geometry, the tree
round trip through load_sixd / the PNG decoder / annotate_sequence, the two training loaders and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import raster_common as rc  # noqa: E402
import synth_common as sc  # noqa: E402
from betapose_amd import annotate as A, metrics, sixd, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------- restatement of DESIGN.md 3.15
def u64(a):
    return np.asarray(a, dtype=np.uint64)


def fmix(h):
    h = u64(h)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & M32
    return h ^ (h >> np.uint64(16))


def absorb(h, k):
    return (fmix(u64(h) ^ u64(k)) + np.uint64(0x9E3779B9)) & M32


def image_key(seed, stream, image):
    return absorb(absorb(absorb(0x243F6A88, seed), stream), image)


def draw(key, pixel, channel):
    return fmix(absorb(absorb(key, pixel), channel))


def noise_value(key, pixel, channel):
    """12 bytes of three draws, minus 1530."""
    s = np.zeros(np.shape(pixel), np.int64) - 1530
    for j in range(3):
        d = draw(key, pixel, channel + 3 * j)
        for b in range(4):
            s = s + ((d >> np.uint64(8 * b)) & np.uint64(255)).astype(np.int64)
    return s


def np_background(images, size, seed, first):
    H, W = size
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((images, H, W, 3), np.uint8)
    for i in range(images):
        pk, lk = image_key(seed, 2, first + i), image_key(seed, 1, first + i)
        w = [(int(draw(pk, o, 0)) & 255) + 1 >> o for o in range(4)]
        amp = 64 + (int(draw(pk, 9, 0)) & 127)
        for c in range(3):
            base = int(draw(pk, 8, c)) & 255
            total = np.zeros((H, W), np.int64)
            for o in range(4):
                sh = 6 - o
                gx, gy = xs >> sh, ys >> sh
                fx, fy = (xs & ((1 << sh) - 1)) << (8 - sh), (ys & ((1 << sh) - 1)) << (8 - sh)
                lat = lambda ax, ay: (draw(lk, u64(o << 28) | (u64(ay) << np.uint64(14)) | u64(ax), c) & np.uint64(255)).astype(np.int64)
                q16 = ((256 - fx) * (256 - fy) * lat(gx, gy) + fx * (256 - fy) * lat(gx + 1, gy) + (256 - fx) * fy * lat(gx, gy + 1)
                       + fx * fy * lat(gx + 1, gy + 1))
                total += w[o] * ((q16 + 128) >> 8)
            t = total // sum(w)
            out[i, :, :, c] = np.clip(base + (((t - 32640) * amp + 16384) >> 15), 0, 255)
    return out


def window_coord(x, W, w):
    return np.clip(((2 * x.astype(np.int64) + 1) * w * 32768) // W - 32768, 0, (w - 1) << 16)


def np_windows(bank, windows, size):
    H, W = size
    out = np.zeros((len(windows), H, W, 3), np.uint8)
    for i, (b, x0, y0, w, h, flip) in enumerate(windows.tolist()):
        xs = np.arange(W)
        u, v = window_coord(W - 1 - xs if flip else xs, W, w), window_coord(np.arange(H), H, h)
        ix, iy, fx, fy = u >> 16, v >> 16, ((u & 65535) >> 8)[None, :, None], ((v & 65535) >> 8)[:, None, None]
        ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
        src = bank[b].astype(np.int64)
        tap = lambda ay, ax: src[(y0 + ay)[:, None], (x0 + ax)[None, :]]
        out[i] = ((256 - fx) * (256 - fy) * tap(iy, ix) + fx * (256 - fy) * tap(iy, ix1) + (256 - fx) * fy * tap(iy1, ix)
                  + fx * fy * tap(iy1, ix1) + 32768) >> 16
    return out


BINOMIAL = {0: [1], 1: [1, 2, 1], 2: [1, 4, 6, 4, 1]}


def np_blur_pass(img, r, axis):
    if r == 0:
        return img
    pad = [(0, 0)] * img.ndim
    pad[axis] = (r, r)
    p = np.pad(img, pad, mode="edge")
    n = img.shape[axis]
    s = sum(wk * np.take(p, np.arange(k, k + n), axis=axis) for k, wk in enumerate(BINOMIAL[r]))
    return (s + (1 << (2 * r - 1))) >> (2 * r)


def np_compose(bg, color, depth, params, seed, first):
    I, H, W = depth.shape
    out = np.zeros((I, H, W, 3), np.uint8)
    pixel = np.arange(H * W).reshape(H, W)
    for i in range(I):
        feather, r = int(params[i, 0]), int(params[i, 1])
        m = depth[i] > 0
        mp = np.pad(m.astype(np.int64), 1, mode="edge")
        a = sum(mp[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) if feather else np.full((H, W), 9, np.int64)
        F, B = color[i].astype(np.int64), bg[i].astype(np.int64)
        pasted = np.where(m[..., None], (a[..., None] * F + (9 - a[..., None]) * B + 4) // 9, B)
        v = np_blur_pass(np_blur_pass(pasted, r, 1), r, 0)          # rows first: along x, then along y
        key = image_key(seed, 0, first + i)
        for c in range(3):
            x = ((int(params[i, 2 + c]) * v[..., c] + 128) >> 8) + int(params[i, 5 + c])
            if params[i, 8]:
                x = x + ((noise_value(key, pixel, c) * int(params[i, 8]) + 32768) >> 16)
            out[i, :, :, c] = np.clip(x, 0, 255)
    return out


def np_counts(depth, scale):
    q = np.floor(depth.astype(np.float64) / scale + 0.5)
    return np.where(depth > 0, np.minimum(q, 65535), 0).astype(np.int64)


def np_edges(counts):
    H, W = counts.shape[-2:]
    p = np.pad(counts, [(0, 0)] * (counts.ndim - 2) + [(1, 1), (1, 1)], mode="edge")
    nb = np.stack([p[..., dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return nb.max(0) - nb.min(0)


def np_sensor(depth, scale, params, seed, first):
    I, H, W = depth.shape
    out = np.zeros((I, H, W), np.uint16)
    pixel = np.arange(H * W).reshape(H, W)
    for i in range(I):
        noise_k, edge, p = (int(v) for v in params[i])
        c = np_counts(depth[i], scale)
        v = c.copy()
        if noise_k:
            sigma = (noise_k * c * c) >> 20
            v = v + ((noise_value(image_key(seed, 3, first + i), pixel, 0) * sigma + 32768) >> 16)
        v = np.clip(v, 0, 65535)
        hole = (np_edges(c) > edge) & ((draw(image_key(seed, 4, first + i), pixel, 0) & np.uint64(255)).astype(np.int64) < p)
        out[i] = np.where((c == 0) | hole, 0, v)
    return out


# ---------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("size", sc.SIZES)
def test_background_equals_its_restatement(size):
    got = sc.host_background(size)
    assert np.array_equal(got, np_background(3, size, sc.SEED, 7))
    assert got.std() > 4 and len({got[i].tobytes() for i in range(3)}) == 3     # a texture, and another one per scene


@pytest.mark.parametrize("size", sc.SIZES)
def test_windows_equal_their_restatement(size):
    assert np.array_equal(sc.host_windows(size), np_windows(sc.bank(), sc.WINDOWS, size))


def test_a_window_of_the_output_size_is_a_copy():
    b = sc.bank()
    w = np.array([[1, 4, 2, 40, 30, 0], [1, 4, 2, 40, 30, 1]], np.int32)
    out = synth.background_windows(b, w, (30, 40))
    assert np.array_equal(out[0], b[1, 2:32, 4:44]) and np.array_equal(out[1], b[1, 2:32, 4:44][:, ::-1])
    with pytest.raises(Exception, match="inside"):
        synth.background_windows(b, np.array([[0, 20, 0, 40, 30, 0]], np.int32), (30, 40))


@pytest.mark.parametrize("r,feather", sc.COMPOSE_CASES)
@pytest.mark.parametrize("size", sc.SIZES)
def test_compose_equals_its_restatement(size, r, feather):
    color, depth = sc.scene_stack(size)
    want = np_compose(sc.backgrounds(size), color, depth, sc.compose_table(r, feather), sc.SEED, 7)
    assert np.array_equal(sc.host_compose(size, r, feather), want)


def test_compose_tall_image_equals_its_restatement():
    color, depth = sc.scene_stack(sc.TALL)
    table = sc.compose_table(2, 1)
    got = synth.compose(sc.backgrounds(sc.TALL), color, depth, table, sc.SEED, 7)
    assert np.array_equal(got, np_compose(sc.backgrounds(sc.TALL), color, depth, table, sc.SEED, 7))


@pytest.mark.parametrize("size", sc.SIZES)
def test_sensor_depth_equals_its_restatement(size):
    assert np.array_equal(sc.host_sensor(size), np_sensor(sc.scene_stack(size)[1], sc.DEPTH_SCALE, sc.SENSOR_ROWS, sc.SEED, 7))


# -------------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("size", sc.SIZES)
def test_neutral_compose_is_the_overlay_paste(size):
    color, depth = sc.scene_stack(size)
    bg = sc.backgrounds(size)
    got = synth.compose(bg, color, depth, synth.compose_params(sc.IMAGES, feather=0), sc.SEED)
    assert np.array_equal(got, metrics.overlay(bg, color, depth, alpha=256))


@pytest.mark.parametrize("r", [1, 2])
def test_blur_keeps_a_constant_and_spreads_an_impulse_by_the_binomial_weights(r):
    H, W = 9, 11
    none = np.zeros((1, H, W), np.float32)
    const = np.full((1, H, W, 3), 201, np.uint8)
    p = synth.compose_params(1, blur=r)
    assert np.array_equal(synth.compose(const, const, none, p, 0), const)
    imp = np.zeros((1, H, W, 3), np.uint8)
    imp[0, 4, 5] = 255
    got = synth.compose(imp, imp, none, p, 0)[0, :, :, 0].astype(np.int64)
    w = np.array(BINOMIAL[r])
    rows = (255 * w + (1 << (2 * r - 1))) >> (2 * r)                        # the row pass, rounded half up
    want = (w[:, None] * rows[None, :] + (1 << (2 * r - 1))) >> (2 * r)     # the column pass over its result
    assert np.array_equal(got[4 - r:5 + r, 5 - r:6 + r], want)
    assert got.sum() == want.sum()
    assert {1: [64, 128, 64], 2: [16, 64, 96, 64, 16]}[r] == rows.tolist()


# -------------------------------------------------------------------------------------------------- noise statistics
def test_noise_mean_and_variance_are_irwin_halls():
    """The noise value is a sum of 12 independent uniform bytes minus 1530: its exact distribution is the 12-fold
    convolution of the uniform law on 0 .. 255 (mean 0, variance 12 (256^2 - 1) / 12 = 65 535).  With sigma = 8 grey
    levels (Q8: 2048) the added value is (n 2048 + 32768) >> 16 = floor(n / 32 + 1/2), at most 48 in size, so a grey of
    128 never clamps.  Its exact mean mu, variance s2 and fourth central moment m4 follow from that distribution by
    summation; over N = 64 x 64 x 3 = 12 288 independent samples the sample mean has the standard error sqrt(s2 / N)
    and the sample variance sqrt((m4 - s2^2) / N) (the variance of (x - mu)^2 over N; the N - 1 correction is below
    1e-4 of it).  The sample mean must lie within 4 standard errors of 0 and the sample variance within 4 of s2.
    (mu itself is not 0 but 1/64: n / 32 is a tie once in 32 values and half-up rounding lifts each tie by 1/2; that is
    0.2 standard errors here, and the bound is taken about 0 all the same.)"""
    pmf = np.ones(1)
    for _ in range(12):
        pmf = np.convolve(pmf, np.full(256, 1.0 / 256))
    n = np.arange(len(pmf)) - 1530
    assert abs((pmf * n).sum()) < 1e-9 and abs((pmf * n * n).sum() - synth.NOISE_VARIANCE) < 1e-6
    sigma_q8 = 2048
    added = (n * sigma_q8 + 32768) >> 16
    assert np.abs(added).max() <= 48
    mu = (pmf * added).sum()
    s2 = (pmf * (added - mu) ** 2).sum()
    m4 = (pmf * (added - mu) ** 4).sum()
    assert abs(mu - 1 / 64) < 1e-6 and abs(s2 - (64.0 * 65535 / 65536 + 1 / 12)) < 0.01     # sigma^2 plus the rounding's 1/12
    grey = np.full((1, 64, 64, 3), 128, np.uint8)
    frame = synth.compose(grey, grey, np.zeros((1, 64, 64), np.float32), synth.compose_params(1, sigma=sigma_q8), 12345)
    x = frame.astype(np.float64) - 128
    N = x.size
    assert frame.min() > 0 and frame.max() < 255
    print("mean %.4f (se %.4f), variance %.3f (exact %.3f, se %.3f)" % (x.mean(), np.sqrt(s2 / N), x.var(), s2, np.sqrt((m4 - s2 * s2) / N)))
    assert abs(x.mean()) <= 4 * np.sqrt(s2 / N)
    assert abs(x.var() - s2) <= 4 * np.sqrt((m4 - s2 * s2) / N)
    # the three channels and neighbouring pixels draw different values
    assert not np.array_equal(frame[..., 0], frame[..., 1]) and not np.array_equal(frame[0, :, 1:], frame[0, :, :-1])


# ------------------------------------------------------------------------------------------------------ sensor depth
@pytest.mark.parametrize("size", sc.SIZES)
def test_sensor_depth_without_noise_and_holes_is_the_rounded_depth(size):
    depth = sc.scene_stack(size)[1]
    got = synth.sensor_depth(depth, sc.DEPTH_SCALE, synth.sensor_params(sc.IMAGES), sc.SEED)
    assert np.array_equal(got, np.where(depth > 0, np.floor(depth.astype(np.float64) / sc.DEPTH_SCALE + 0.5), 0).astype(np.uint16))
    assert np.array_equal(got[0], sc.host_sensor(size)[0])                  # SENSOR_ROWS' first row is this sensor
    far = synth.sensor_depth(np.array([[[70.0, 65.5349, 65.5351, 0.0, -1.0]]], np.float32), 0.001, synth.sensor_params(1), 0)
    assert far.tolist() == [[[65535, 65535, 65535, 0, 0]]]                  # clamped; nothing stays nothing


@pytest.mark.parametrize("size", sc.SIZES)
def test_holes_occur_only_on_edges_and_everywhere_on_them_at_p_256(size):
    depth = sc.scene_stack(size)[1]
    counts = np_counts(depth, sc.DEPTH_SCALE)
    edge = 10
    on_edge = (np_edges(counts) > edge) & (counts > 0)
    assert on_edge.any() and (~on_edge & (counts > 0)).any()
    half = synth.sensor_depth(depth, sc.DEPTH_SCALE, synth.sensor_params(sc.IMAGES, 0, edge, 128), sc.SEED)
    holes = (half == 0) & (counts > 0)
    assert holes.any() and not (holes & ~on_edge).any() and (on_edge & ~holes).any()
    assert np.array_equal(half[~holes], counts[~holes].astype(np.uint16))
    assert 0.35 < holes.sum() / on_edge.sum() < 0.65
    every = synth.sensor_depth(depth, sc.DEPTH_SCALE, synth.sensor_params(sc.IMAGES, 0, edge, 256), sc.SEED)
    assert np.array_equal((every == 0) & (counts > 0), on_edge)


# ---------------------------------------------------------------------------------------------------------- chunking
def test_three_scenes_in_one_call_equal_three_calls():
    size = sc.SIZES[1]
    color, depth = sc.scene_stack(size)
    bg = sc.backgrounds(size)
    table, rows = sc.compose_table(2, 1), sc.SENSOR_ROWS
    whole = (synth.procedural_background(3, size, 5, 0), synth.compose(bg[:3], color[:3], depth[:3], table[:3], 5, 0),
             synth.sensor_depth(depth[:3], sc.DEPTH_SCALE, rows[1:4], 5, 0))
    for i in range(3):
        s = slice(i, i + 1)
        assert np.array_equal(synth.procedural_background(1, size, 5, i), whole[0][s])
        assert np.array_equal(synth.compose(bg[s], color[s], depth[s], table[s], 5, i), whole[1][s])
        assert np.array_equal(synth.sensor_depth(depth[s], sc.DEPTH_SCALE, rows[1 + i:2 + i], 5, i), whole[2][s])
    # and the scene number matters: the same inputs as another scene give other noise
    assert not np.array_equal(synth.compose(bg[1:2], color[1:2], depth[1:2], table[1:2], 5, 0), whole[1][1:2])


# ---------------------------------------------------------------------------------------------------------- geometry
def test_sample_poses_keep_their_ranges():
    size, K, radius = (75, 113), rc.camera((75, 113)), 0.05
    kw = dict(elevation=(15.0, 70.0), distance=(0.4, 0.9), inplane=(-45.0, 45.0), margin=9.0)
    poses = synth.sample_poses(200, K, size, radius, 4, **kw)
    assert poses.shape == (200, 3, 4)
    R, t = poses[:, :, :3], poses[:, :, 3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(R) - 1).max() < 1e-12
    u, v = K[0, 0] * t[:, 0] / t[:, 2] + K[0, 2], K[1, 1] * t[:, 1] / t[:, 2] + K[1, 2]
    assert u.min() >= 9 - 1e-9 and u.max() <= 112 - 9 + 1e-9 and v.min() >= 9 - 1e-9 and v.max() <= 74 - 9 + 1e-9
    dist = np.linalg.norm(t, axis=1)
    assert dist.min() >= 0.4 - 1e-12 and dist.max() <= 0.9 + 1e-12
    cam = -np.einsum("nji,nj->ni", R, t)                                    # the camera's centre in the object's frame
    el = np.degrees(np.arcsin(cam[:, 2] / dist))
    assert el.min() >= 15 - 1e-9 and el.max() <= 70 + 1e-9
    assert u.std() > 10 and el.std() > 5 and dist.std() > 0.05             # and they do vary
    again = synth.sample_poses(200, K, size, radius, 4, **kw)
    assert again.tobytes() == poses.tobytes()
    assert synth.sample_poses(3, K, size, radius, 4, first_scene=7, **kw).tobytes() == poses[7:10].tobytes()
    assert synth.sample_poses(3, K, size, radius, 5, **kw).tobytes() != poses[:3].tobytes()
    assert synth.sample_poses(0, K, size, radius, 4, **kw).shape == (0, 3, 4)


def test_occluders_lie_between_camera_and_target():
    size, K = (75, 113), rc.camera((75, 113))
    tp = synth.sample_poses(50, K, size, 0.05, 4)
    occ = synth.place_occluders(tp, 0.05, K, size, 4, 3, depth_fraction=(0.3, 0.8), lateral=1.5)
    assert occ.shape == (50, 3, 3, 4)
    t = tp[:, None, :, 3]
    along = (occ[..., 3] * t).sum(-1) / np.linalg.norm(t, axis=-1)          # the centre's distance along the target's ray
    dist = np.linalg.norm(t, axis=-1)
    assert (along > 0).all() and (along < dist).all()
    assert (along >= 0.3 * dist - 1e-12).all() and (along <= 0.8 * dist + 1e-12).all()
    side = np.linalg.norm(occ[..., 3] - along[..., None] * t / dist[..., None], axis=-1)
    assert side.max() <= 1.5 * 0.05 + 1e-12 and side.max() > 0.05
    R = occ[..., :3]
    assert np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(R) - 1).max() < 1e-12
    assert synth.place_occluders(tp, 0.05, K, size, 4, 3, stream=1).tobytes() != synth.place_occluders(tp, 0.05, K, size, 4, 3).tobytes()


# -------------------------------------------------------------------------------------------------------- round trip
@pytest.fixture(scope="module")
def scenes():
    return sc.synthesize(4)


@pytest.fixture(scope="module")
def tree(scenes, tmp_path_factory):
    base = str(tmp_path_factory.mktemp("synth_tree"))
    synth.write_scene_tree(base, 1, scenes, sc.scene_meshes(), rc.camera(sc.SCENES_SIZE), 0.001)
    return base


def test_scenes_are_what_they_say(scenes):
    H, W = sc.SCENES_SIZE
    assert scenes["frames"].shape == (4, H, W, 3) and scenes["depth"].shape == (4, H, W) and scenes["depth"].dtype == np.uint16
    assert scenes["poses"].shape == (4, 2, 3, 4) and scenes["obj_ids"].tolist() == [1, 2]
    assert np.array_equal(scenes["poses"][..., 3], scenes["t_mm"] * 0.001)
    vf = scenes["visib_fract"]
    assert ((vf > 0) & (vf < 1)).any(), vf                                  # the occluder does hide something: seed's choice
    assert (vf[scenes["present"][:, 1]] >= 0.3).all()
    # chunks concatenate to the whole
    for key, whole in scenes.items():
        if key != "obj_ids":
            parts = np.concatenate([sc.synthesize(2)[key], sc.synthesize(2, first_scene=2)[key]])
            assert np.array_equal(parts, whole), key


def test_redraws_end_without_occluders():
    """min_visib above 1 can never be met: every scene runs out of redraws and keeps no occluder."""
    m = sc.scene_meshes()
    metres = lambda mesh: (mesh[0] * 0.001, mesh[1], mesh[2])
    s = synth.synthesize_scenes(metres(m[1]), [metres(m[2])], rc.camera(sc.SCENES_SIZE), sc.SCENES_SIZE, 2, sc.SCENES_SEED,
                                min_visib=1.5, max_redraws=2, sensor=dict(noise_k=0, hole_p=0))
    assert s["redraws"].tolist() == [3, 3] and not s["present"][:, 1].any() and s["present"][:, 0].all()
    assert (s["visib_fract"] == 1.0).all() and (s["box_full"][:, 1] == -1).all()


def test_tree_round_trip(scenes, tree):
    bench = sixd.load_sixd(tree, 1, load_depth=True)
    assert np.array_equal(bench.cam, rc.camera(sc.SCENES_SIZE)) and len(bench.frames) == 4
    for i, fr in enumerate(bench.frames):
        present = [j for j in range(2) if scenes["present"][i, j]]
        assert [g[0] for g in fr.gt] == [int(scenes["obj_ids"][j]) for j in present] and fr.gt[0][0] == 1
        for g, j in zip(fr.gt, present):
            assert g[1][:3].tobytes() == scenes["poses"][i, j].tobytes()     # rotation bits, and t_mm * 0.001 bits
            xmin, xmax, ymin, ymax = scenes["box_full"][i, j]
            assert list(g[2]) == [xmin, ymin, xmax - xmin, ymax - ymin]
        assert np.array_equal(fr.depth, scenes["depth"][i]) and np.array_equal(fr.cam, bench.cam)
        from betapose_amd.frame_loader import decode_png
        with open(os.path.join(tree, "test", "01", "rgb", "%04d.png" % i), "rb") as f:
            assert np.array_equal(decode_png(f.read()), scenes["frames"][i])     # BGR, as the loaders read it
    v, f, c = metrics.load_ply_colored_mesh(os.path.join(tree, "models", "obj_01.ply"))
    m = sc.scene_meshes()[1]
    assert v.tobytes() == np.ascontiguousarray(m[0]).tobytes() and np.array_equal(f, m[1]) and np.array_equal(c, m[2])
    assert abs(bench.diameter[1] - rc.diameter(m[0])) < 1e-9


def test_annotator_agrees_with_the_synthesiser(scenes, tree):
    bench = sixd.load_sixd(tree, 1, load_depth=True)
    v, f = metrics.load_ply_mesh(os.path.join(tree, "models", "obj_01.ply"))
    model = metrics.Model3D()
    model.vertices = v * bench.scale_to_meters
    bench.models["01"] = model
    kp3d = model.vertices[::5]
    ann = A.annotate_sequence(bench, 1, kp3d, f, use_depth=True, size=sc.SCENES_SIZE)
    assert np.array_equal(ann["box_full"], scenes["box_full"][:, 0])
    bb = np.array([fr.gt[0][2] for fr in bench.frames])
    assert np.array_equal(ann["box_full"], np.stack([bb[:, 0], bb[:, 0] + bb[:, 2], bb[:, 1], bb[:, 1] + bb[:, 3]], axis=1))
    assert np.array_equal(ann["box_visible"], scenes["box_visible"])
    assert np.array_equal(ann["visib_fract"], scenes["visib_fract"])


# ----------------------------------------------------------------------------------------------------------- loaders
def test_exported_training_set_feeds_both_loaders(scenes, tree, tmp_path):
    from betapose_amd.train_data import KPDSampleLoader
    from betapose_amd.yolo_train import YoloSampleLoader
    bench = sixd.load_sixd(tree, 1, load_depth=True)
    v, f = metrics.load_ply_mesh(os.path.join(tree, "models", "obj_01.ply"))
    model = metrics.Model3D()
    model.vertices = v * bench.scale_to_meters
    bench.models["01"] = model
    ann = A.annotate_sequence(bench, 1, model.vertices[::5], f, use_depth=True, size=sc.SCENES_SIZE)
    annot = str(tmp_path / "annot")
    A.write_annotations(annot, ann, 3, image_size=sc.SCENES_SIZE)
    lists = synth.export_training_set(tree, annot, str(tmp_path / "set"))
    Kp = len(model.vertices[::5])
    kpd = KPDSampleLoader(os.path.join(annot, "annot_train.npz"), str(tmp_path / "set" / "kpd"), batch=4, train=False,
                          in_res=(64, 48), out_res=(16, 12), threads=1)
    batches = list(kpd)
    assert len(batches) == 1
    inps, labels, mask = batches[0]
    assert inps.shape == (3, 3, 64, 48) and labels.shape == (3, Kp, 16, 12) and len(mask) == 3
    det = YoloSampleLoader(lists["train"], batch=4, net_size=(96, 96), train=False, threads=1)
    batches = list(det)
    assert len(batches) == 1
    inps, truth = batches[0]
    assert inps.shape == (3, 3, 96, 96) and truth.shape == (3, 90, 5)
    H, W = sc.SCENES_SIZE
    with open(lists["train"]) as fl:
        paths = [ln.strip() for ln in fl]
    for k, p in enumerate(paths):
        with open(p[:-4] + ".txt") as fl:
            line = [float(t) for t in fl.read().split()]
        x1, y1, x2, y2 = ann["bbox"][list(ann["frames"]).index(int(os.path.basename(p)[:-4]))]
        assert np.allclose(line, [0, (x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H], atol=1e-6)
        assert np.allclose(truth[k, 0], [line[1], line[2], line[3], line[4], 0], atol=1e-6) and not truth[k, 1:].any()


# --------------------------------------------------------------------------------------------------------------- CLI
def test_command_line_writes_the_tree_twice_alike(tmp_path):
    m = sc.scene_meshes()
    ply = str(tmp_path / "obj_01.ply")
    occ = str(tmp_path / "occ.ply")
    synth._write_mesh_ply(ply, m[1][0], m[1][1], m[1][2])
    synth._write_mesh_ply(occ, m[2][0], m[2][1])
    trees = []
    for name in ("a", "b"):
        out = str(tmp_path / name)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "synthesize.py"), "--model", ply, "--occluders", occ, "--obj_id", "1",
                            "--frames", "3", "--out", out, "--size", "48x64", "--camera", "60,60,31.5,23.5", "--seed", "3"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        files = {}
        for dirpath, _, names in os.walk(out):
            for n in names:
                with open(os.path.join(dirpath, n), "rb") as f:
                    files[os.path.relpath(os.path.join(dirpath, n), out)] = f.read()
        trees.append(files)
    want = {"camera.yml", "models/models_info.yml", "models/obj_01.ply", "models/obj_02.ply", "test/01/gt.yml", "test/01/info.yml"}
    want |= {"test/01/%s/%04d.png" % (d, i) for d in ("rgb", "depth") for i in range(3)}
    assert set(trees[0]) == want
    assert trees[0] == trees[1]
    bench = sixd.load_sixd(str(tmp_path / "a"), 1, load_depth=True)
    assert len(bench.frames) == 3 and bench.frames[0].gt[0][0] == 1 and bench.frames[0].depth.shape == (48, 64)
