"""The key-point designator's host twins (betapose_amd/designate.py with device=None; csrc/designate_host.cpp) against
the definitions of DESIGN.md 3.9, restated in numpy in designate_common.py, and against metrics.refine_keypoints.  No
GPU is needed."""
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import designate_common as dc
from betapose_amd import _lib, designate as D, metrics

ROOT = dc.ROOT


def _pair_G(s, sigma=1.0):
    """G_1 at the first of two points (0, 0, 0), (s, 0, 0) on the field x: scale 0 is too narrow to reach the second
    point, so G_0 = 0 exactly and DoG[0] = G_1 = s w / (1 + w)."""
    pts = np.array([[0.0, 0.0, 0.0], [s, 0.0, 0.0]])
    dog, _ = D.sift_octave(pts, 0, [0.005, sigma, sigma, sigma], k=2)
    return dog[0, 0]


def test_ds_exp_through_a_two_point_cloud():
    worst = 0.0
    for t in np.linspace(0.0, 1.0, 10001):
        s = 3.0 * math.sqrt(t)                          # the argument -s^2 / 2 covers [-4.5, 0] evenly
        w = math.exp((-0.5 * (s * s)) / 1.0)
        want = s * w / (1.0 + w)
        got = _pair_G(s)
        if want == 0.0:
            assert got == 0.0
        else:
            worst = max(worst, abs(got - want) / want)
    print("largest relative error of G over 10001 spacings: %.3g" % worst)
    assert worst <= 1e-14


def test_cutoff_is_inclusive_at_exactly_nine_sigma_squared():
    inside, outside = _pair_G(3.0), _pair_G(np.nextafter(3.0, 4.0))
    w = math.exp(-4.5)
    assert abs(inside - 3.0 * w / (1.0 + w)) <= 1e-14 * inside
    assert outside == 0.0


@pytest.mark.parametrize("octave", [0, 1, 2])
def test_dog_equals_the_numpy_oracle_and_flags_follow_from_it(octave):
    cloud, scales = dc.octave_clouds()[octave]
    assert len(cloud) == dc.OCTAVE_SIZES[octave]
    dog, flags = D.sift_octave(cloud, 2, scales, k=25, min_contrast=0.02)
    want = dc.dog_oracle(cloud, 2, scales)
    err = np.abs(dog - want).max()
    print("octave %d: max |DoG - oracle| = %.3g, max |field| = %.3g" % (octave, err, np.abs(cloud[:, 2]).max()))
    assert err <= 1e-12 * np.abs(cloud[:, 2]).max()
    assert np.array_equal(flags, dc.flags_oracle(cloud, dog, 25, 0.02))
    assert (flags != 0).any()


def test_flags_with_more_neighbours_than_points_and_duplicates():
    pts = dc.with_duplicates(300)
    scales = D.octave_scales(1.0, 0, 3)
    dog, flags = D.sift_octave(pts, 2, scales, k=25, min_contrast=0.02)
    assert np.array_equal(flags, dc.flags_oracle(pts, dog, 25, 0.02))
    small = dc.nearest_part(30)
    dog, flags = D.sift_octave(small, 2, scales, k=40, min_contrast=0.0)
    assert np.array_equal(flags, dc.flags_oracle(small, dog, 40, 0.0))


def test_scene_key_points_sit_on_the_bumps():
    kp, sizes = D.sift_keypoints(dc.scene(), min_contrast=0.2, return_sizes=True, **dc.SCENE_ARGS)
    assert sizes == dc.OCTAVE_SIZES
    assert kp.shape[1] == 6 and len(kp) >= 3
    centres = np.array([b[:2] for b in dc.BUMPS])
    dist = np.hypot(kp[:, None, 0] - centres[None, :, 0], kp[:, None, 1] - centres[None, :, 1])      # [kp, bump]
    for b, (_, _, h, s) in enumerate(dc.BUMPS):
        near = dist[:, b] <= s
        assert near.any(), "no key point within sigma of bump %d" % b
        assert (kp[near, 5] == (-1.0 if h > 0 else 1.0)).all()
    assert (dist.min(axis=1) <= 3.0).all()
    many = D.sift_keypoints(dc.scene(), min_contrast=0.02, **dc.SCENE_ARGS)
    assert len(many) > len(kp) and set(many[:, 4]) == {0.0, 1.0, 2.0} and set(many[:, 5]) == {-1.0, 1.0}
    # the rows are (point, scale) ordered within an octave, and the scale column is one of the octave's inner scales
    for o in range(3):
        inner = dc.octave_clouds()[o][1][1:-2]
        assert np.isin(many[many[:, 4] == o, 3], inner).all()


def test_voxel_grid():
    pts = dc.scene()
    out = D.voxel_grid(pts, 2.0)
    cell = np.floor(pts / 2.0).astype(np.int64)
    lo = cell.min(axis=0)
    d = cell.max(axis=0) - lo + 1
    key = (cell[:, 0] - lo[0]) + (cell[:, 1] - lo[1]) * d[0] + (cell[:, 2] - lo[2]) * d[0] * d[1]
    keys = np.unique(key)
    assert len(out) == len(keys)
    want = np.empty((len(keys), 3))
    for r, kv in enumerate(keys):                      # ascending key; summed in ascending input index
        acc = np.zeros(3)
        rows = np.flatnonzero(key == kv)
        for i in rows:
            acc = acc + pts[i]
        want[r] = acc / len(rows)
    assert np.array_equal(out, want)
    # a negative coordinate floors downwards
    two = D.voxel_grid(np.array([[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0], [0.7, 0.0, 0.0]]), 1.0)
    assert np.array_equal(two, np.array([[-0.5, 0.0, 0.0], [(0.5 + 0.7) / 2.0, 0.0, 0.0]]))
    # more cells than INT32_MAX: the cloud passes through unchanged
    assert np.array_equal(D.voxel_grid(pts, 1e-6), pts)


def _thin_equals_refine(pts, keep):
    try:
        want = metrics.refine_keypoints(pts, keep)
    except IndexError:                                  # (the carried position ran off the end: so must ours)
        with pytest.raises(IndexError):
            D.thin_points(pts, keep)
        return None
    got = np.asarray(pts)[D.thin_points(pts, keep)]
    assert got.shape == want.shape and np.array_equal(got, want)
    return got


def test_thin_points_equals_refine_keypoints():
    v = metrics.load_ply_vertices(os.path.join(ROOT, "tests", "golden", "sifts_1.ply"))
    assert len(v) == 50
    assert len(_thin_equals_refine(v, 30)) == 30
    _thin_equals_refine(v, 50)
    _thin_equals_refine(v, 60)
    _thin_equals_refine(v, 1)
    pts = dc.thin_cloud(120)
    _thin_equals_refine(pts, 30)
    _thin_equals_refine(pts * 40.0, 30)                 # spread out: the 100.0 cap is reached after the duplicates


def test_thin_points_keeps_the_references_quirks():
    far = dc.far_cloud(10)
    got = _thin_equals_refine(far, 6)                   # no pair below 100: position 0 is deleted four times
    assert np.array_equal(got, far[4:])
    close = np.array(far)
    close[9] = close[8] + [1.0, 0.0, 0.0]               # one close pair at rows 8, 9: row 8 goes, then position 8 again
    assert np.array_equal(_thin_equals_refine(close, 8), close[:8])
    with pytest.raises(IndexError):
        metrics.refine_keypoints(close, 7)
    with pytest.raises(IndexError):
        D.thin_points(close, 7)
    # the closed form of the tail against numpy's delete, round by round
    for L, R, m in ((10, 3, 0), (10, 3, 7), (10, 3, 8), (10, 1, 9), (10, 1, 10), (5, 0, 9), (6, 6, 0), (6, 4, 3)):
        rows = np.arange(L)
        try:
            want = rows
            for _ in range(R):
                want = np.delete(want, m, axis=0)
        except IndexError:
            with pytest.raises(IndexError):
                D.thin_tail(rows, R, m)
            continue
        assert np.array_equal(D.thin_tail(rows, R, m), want)


def test_farthest_points_equals_the_numpy_loop():
    for pts, K, start in ((dc.with_duplicates(300), 50, None), (dc.nearest_part(65), 65, None), (dc.with_duplicates(300), 8, 17),
                          (dc.nearest_part(30), 1, None)):
        idx, d2 = D.farthest_points(pts, K, start)
        want_idx, want_d2 = dc.fps_oracle(pts, K, start)
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(d2, want_d2)
    # all 65 of 65 points: a permutation; one more round than there are distinct points picks a distance of 0
    idx, d2 = D.farthest_points(dc.nearest_part(65), 65)
    assert sorted(idx) == list(range(65)) and (d2[1:] > 0).all()
    idx, d2 = D.farthest_points(dc.with_duplicates(300), 300)
    assert (d2[-3:] == 0.0).all() and (d2[1:-3] > 0).all()


def _cli():
    spec = importlib.util.spec_from_file_location("designate_cli", os.path.join(ROOT, "designate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_round_trip(tmp_path, capsys):
    model = str(tmp_path / "models" / "obj_01.ply")
    D.write_ply(model, dc.scene())
    head = open(model).read().split("\n")[:8]
    assert head[:7] == ["ply", "format ascii 1.0", "element vertex 1681", "property float x", "property float y",
                        "property float z", "end_header"]
    assert head[7].endswith(" ") and len(head[7].split()) == 3
    sift = ["--min_scale", "1.0", "--n_octaves", "3", "--n_scales_per_octave", "3", "--min_contrast", "0.02"]
    out = str(tmp_path / "kpmodels" / "obj_01.ply")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "designate.py"), "--model", model, "--output", out,
                        "--total_kp_number", "5"] + sift, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "# of points in octave 0 are " in r.stdout and "# of key points kept are 5" in r.stdout
    found = int(r.stdout.split("# of SIFT points in the result are ")[1].split()[0])
    assert found > 5
    kp = metrics.load_ply_vertices(out)
    assert kp.shape == (5, 3)
    m = metrics.Model3D(out)
    m.refine(5)
    assert np.array_equal(m.vertices, kp)
    # every key point is a point of an octave cloud, hence inside the model's box
    v = metrics.load_ply_vertices(model)
    assert (kp >= v.min(axis=0) - 1e-4).all() and (kp <= v.max(axis=0) + 1e-4).all()
    # fewer SIFT points than asked for: returned as they are
    cli = _cli()
    out2 = str(tmp_path / "kpmodels" / "all.ply")
    assert cli.main(["--model", model, "--output", out2, "--total_kp_number", "50"] + sift) == 0
    text = capsys.readouterr().out
    assert "# of SIFT points in the result are %d" % found in text and "# of key points kept are %d" % found in text
    assert len(metrics.load_ply_vertices(out2)) == found
    # farthest points
    out3 = str(tmp_path / "kpmodels" / "fps.ply")
    assert cli.main(["--model", model, "--output", out3, "--total_kp_number", "7", "--method", "fps"]) == 0
    fps = metrics.load_ply_vertices(out3)
    want = v[D.farthest_points(v, 7)[0]]
    assert fps.shape == (7, 3) and np.allclose(fps, want, rtol=1e-6, atol=0)


def test_designate_function():
    pts = dc.scene()
    kp, info = D.designate(pts, 5, min_contrast=0.02, return_info=True, **dc.SCENE_ARGS)
    allkp = D.sift_keypoints(pts, min_contrast=0.02, **dc.SCENE_ARGS)
    assert info == {"octave_sizes": dc.OCTAVE_SIZES, "found": len(allkp), "kept": 5}
    assert np.array_equal(kp, metrics.refine_keypoints(allkp[:, :3], 5))
    few = D.designate(pts, 50, min_contrast=0.02, **dc.SCENE_ARGS)
    assert np.array_equal(few, allkp[:, :3])
    assert np.array_equal(D.designate(pts, 9, method="fps"), pts[D.farthest_points(pts, 9)[0]])
    with pytest.raises(ValueError):
        D.designate(pts, 9, method="other")


def test_argument_checks():
    L = _lib.lib()
    pts = np.array(dc.nearest_part(30))
    sc = D.octave_scales(1.0, 0, 3)
    dog, flags = np.empty((30, 5)), np.empty((30, 3), np.int8)
    idx, d2 = np.empty(64, np.int32), np.empty(64)
    alive, state = np.empty(30, np.uint8), np.empty(2, np.int32)
    out, n_out = np.empty((30, 3)), _lib.C.c_int(0)
    P = _lib.ptr

    def octave(n=30, field=2, scales=sc, ns=6, k=25, mc=0.2):
        scales = np.ascontiguousarray(scales, dtype=np.float64)
        return L.bp_sift_octave_host(P(pts), n, field, P(scales), ns, k, mc, P(dog), P(flags))

    assert octave() == 0
    bad = [octave(n=0), octave(n=(1 << 17) + 1), octave(ns=3), octave(ns=13), octave(k=0), octave(k=65), octave(field=3),
           octave(field=-1), octave(mc=-1.0), octave(scales=sc[::-1]), octave(scales=np.r_[0.0, sc[1:]]),
           octave(scales=np.r_[sc[:5], np.inf]),
           L.bp_sift_octave_host(None, 30, 2, P(sc), 6, 25, 0.2, P(dog), P(flags)),
           L.bp_farthest_points_host(P(pts), 0, 1, -1, P(idx), P(d2)),
           L.bp_farthest_points_host(P(pts), 30, 0, -1, P(idx), P(d2)),
           L.bp_farthest_points_host(P(pts), 30, 31, -1, P(idx), P(d2)),
           L.bp_farthest_points_host(P(pts), 30, 5, 30, P(idx), P(d2)),
           L.bp_farthest_points_host(P(pts), (1 << 20) + 1, 5, -1, P(idx), P(d2)),
           L.bp_thin_points_host(P(pts), 0, 5, P(alive), P(state)),
           L.bp_thin_points_host(P(pts), 30, 0, P(alive), P(state)),
           L.bp_thin_points_host(P(pts), (1 << 14) + 1, 5, P(alive), P(state)),
           L.bp_voxel_grid_host(P(pts), 0, 1.0, P(out), _lib.C.byref(n_out)),
           L.bp_voxel_grid_host(P(pts), 30, 0.0, P(out), _lib.C.byref(n_out)),
           L.bp_voxel_grid_host(P(pts), 30, float("nan"), P(out), _lib.C.byref(n_out))]
    assert all(rc == -1 for rc in bad), bad
    assert L.bp_last_error()
    # the device entry points refuse the same sizes before anything is enqueued (no GPU is touched)
    assert L.bp_sift_octave(P(pts), 0, 2, P(sc), 6, 25, 0.2, P(dog), P(flags), None) == -1
    assert L.bp_farthest_points(P(pts), 30, 31, -1, P(idx), P(d2), None) == -1
    assert L.bp_thin_points(P(pts), 30, 0, P(alive), P(state), None) == -1
    # the Python wrappers
    for call in (lambda: D.sift_octave(pts, 2, sc[:3]), lambda: D.sift_octave(pts[:, :2], 2, sc),
                 lambda: D.farthest_points(pts, 5, start=30), lambda: D.sift_keypoints(pts, n_scales_per_octave=10),
                 lambda: D.voxel_grid(np.full((3, 3), np.nan), 1.0), lambda: D.designate(pts, 0)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_lib.BetaposeHipError):
        D.farthest_points(pts, 31)
    with pytest.raises(_lib.BetaposeHipError):
        D.thin_points(pts, 0)
