"""bp_render_depth (csrc/raster.hip) and bp_vsd_errors (csrc/vsd.hip) against their host twins: the depth images as uint32
bit patterns with the skipped counts -- every mesh, pose and edge case of test_raster_host.py, several poses in one call,
repeated calls and a second stream -- the VSD errors and counts exactly, for every chunk size, and the argument checks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raster_common as rc  # noqa: E402

H, W, K = rc.H, rc.W, rc.K
FILL = 7


def device_render(poses, v, f, c=0.0, near=0.01, stream=None, size=(H, W)):
    import torch
    from betapose_amd import _lib
    poses = np.ascontiguousarray(np.asarray(poses, np.float64)[:, :3, :4]).reshape(-1, 12)
    d_model = torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda()
    d_faces = torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()
    d_poses = torch.from_numpy(poses).cuda()
    d_depth = torch.full((len(poses), size[0], size[1]), float(FILL), dtype=torch.float32, device="cuda")
    d_skipped = torch.full((len(poses),), FILL, dtype=torch.int32, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    _lib.check(_lib.lib().bp_render_depth(_lib.ptr(d_model), len(v), _lib.ptr(d_faces), len(f), _lib.ptr(d_poses), len(poses),
                                          _lib.ptr(np.ascontiguousarray(K).reshape(9)), size[0], size[1], c, near,
                                          _lib.ptr(d_depth), _lib.ptr(d_skipped), s.cuda_stream))
    return d_depth.cpu().numpy(), d_skipped.cpu().numpy()


def assert_same_image(got, want):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize("c", [0.0, 0.5])
@pytest.mark.parametrize("name", ["icosphere", "torus", "box"])
def test_render_parity_random_poses(name, c):
    v, f = rc.MESHES[name]()
    assert_same_image(device_render(rc.poses_for(name), v, f, c), rc.host_render(name, c))


@pytest.mark.parametrize("case", ["box_closeup", "half_outside", "outside", "behind_near"])
def test_render_parity_edge_cases(case):
    from betapose_amd import metrics
    v, f, pose, near = rc.edge_cases()[case]
    want = metrics.render_depth(pose[None], v, f, K, (H, W), near=near)
    assert_same_image(device_render(pose[None], v, f, near=near), want)
    assert_same_image(metrics.render_depth(pose[None], v, f, K, (H, W), device="cuda", near=near), want)
    if case == "behind_near":
        assert want[1][0] > 0
    if case == "box_closeup":
        assert (want[0] > 0).mean() > 0.9


def test_render_parity_shared_edge():
    from betapose_amd import metrics
    z = 2.0
    v = np.array([[(u - K[0, 2]) / K[0, 0] * z, (w - K[1, 2]) / K[1, 1] * z, z] for u, w in [(10, 5), (20, 5), (20, 15), (10, 15)]])
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    got = device_render(np.eye(4)[None], v, f)
    assert_same_image(got, metrics.render_depth(np.eye(4)[None], v, f, K, (H, W)))
    want = np.zeros((H, W), bool)
    want[5:15, 10:20] = True
    assert np.array_equal(got[0][0] > 0, want)


def test_render_five_poses_repeats_and_second_stream():
    """P = 5 in one call (the torus' four poses and one more: not a multiple of anything), twice on the current stream and
    once on another: all bit-identical to the host."""
    import torch
    from betapose_amd import metrics
    v, f = rc.torus()
    poses = np.concatenate([rc.poses_for("torus"), rc.poses_for("torus", 6)[5:]])
    assert len(poses) == 5
    want = metrics.render_depth(poses, v, f, K, (H, W))
    first = device_render(poses, v, f)
    assert_same_image(first, want)
    assert_same_image(device_render(poses, v, f), first)
    assert_same_image(device_render(poses, v, f, stream=torch.cuda.Stream()), first)
    torch.cuda.synchronize()


def test_render_bad_face_index_is_skipped_and_counted():
    """The device call cannot refuse an index it has not read: the kernel skips the triangle and counts it."""
    from betapose_amd import metrics
    v, f = rc.box()
    pose = np.eye(4)[None, :3].copy()
    pose[0, 2, 3] = 3.0
    bad = f.copy()
    bad[3, 1], bad[7, 0] = len(v), -1
    depth, skipped = device_render(pose, v, bad)
    assert skipped[0] == 2
    keep = np.ones(len(f), bool)
    keep[[3, 7]] = False
    assert np.array_equal(depth.view(np.uint32), metrics.render_depth(pose, v, f[keep], K, (H, W))[0].view(np.uint32))


# ---------------------------------------------------------------- VSD

def device_vsd(v, f, gt, est, test, index, d, chunk=0, taus=None, stream=None):
    import torch
    from betapose_amd import _lib, metrics
    taus = np.ascontiguousarray(metrics.BOP_VSD_TAUS if taus is None else taus, np.float64)
    P = len(gt)
    d_model = torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda()
    d_faces = torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()
    d_gt = torch.from_numpy(np.ascontiguousarray(gt[:, :3, :4]).reshape(P, 12)).cuda()
    d_est = torch.from_numpy(np.ascontiguousarray(est[:, :3, :4]).reshape(P, 12)).cuda()
    d_test = torch.from_numpy(np.ascontiguousarray(test).view(np.int16)).cuda()
    d_idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).cuda()
    d_err = torch.full((P, len(taus)), float(FILL), dtype=torch.float64, device="cuda")
    d_counts = torch.full((P, 4), FILL, dtype=torch.int32, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    _lib.check(_lib.lib().bp_vsd_errors(_lib.ptr(d_model), len(v), _lib.ptr(d_faces), len(f), _lib.ptr(d_gt), _lib.ptr(d_est), P,
                                        _lib.ptr(np.ascontiguousarray(K).reshape(9)), _lib.ptr(d_test), test.shape[0], H, W,
                                        0.001, _lib.ptr(d_idx), metrics.BOP_VSD_DELTA, _lib.ptr(taus), len(taus), d, 0.0, 0.01,
                                        chunk, _lib.ptr(d_err), _lib.ptr(d_counts), s.cuda_stream))
    return d_err.cpu().numpy(), d_counts.cpu().numpy()


def test_vsd_parity_and_chunks():
    import torch
    from betapose_amd import metrics
    v, f, gt, est, test, index, d = rc.vsd_scene()
    # precondition, from the host's intermediates: no pixel sits within 1e-9 of a threshold, so a last-bit difference in
    # a distance could not move a count
    dg = metrics.render_depth(gt, v, f, K, (H, W))[0]
    de = metrics.render_depth(est, v, f, K, (H, W))[0]
    for p in range(len(gt)):
        m = metrics.vsd_masks(test[index[p]].astype(np.float64) * 0.001, dg[p], de[p], K, metrics.BOP_VSD_DELTA)
        on = m["dist_gt"] > 0
        assert np.abs((m["dist_gt"] - m["dist_test"])[on] - metrics.BOP_VSD_DELTA).min() > 1e-9
        on = m["dist_est"] > 0
        assert np.abs((m["dist_est"] - m["dist_test"])[on] - metrics.BOP_VSD_DELTA).min() > 1e-9
        rel = np.abs(m["dist_gt"] - m["dist_est"])[m["inter"]] / d
        assert np.abs(rel[:, None] - np.asarray(metrics.BOP_VSD_TAUS)[None]).min() > 1e-9
    want_err, want_counts = metrics.pose_errors_vsd(gt, est, v, f, K, test, index, d)
    assert len(np.unique(want_err)) > 10                 # the scene separates the pairs and the taus
    for chunk in (1, 2, 0):
        err, counts = device_vsd(v, f, gt, est, test, index, d, chunk)
        assert np.array_equal(counts, want_counts), chunk
        assert np.array_equal(err, want_err), chunk
    err, counts = device_vsd(v, f, gt, est, test, index, d, 2, stream=torch.cuda.Stream())
    assert np.array_equal(counts, want_counts) and np.array_equal(err, want_err)
    err, counts = metrics.pose_errors_vsd(gt, est, v, f, K, test, index, d, device="cuda", chunk=3)
    assert np.array_equal(counts, want_counts) and np.array_equal(err, want_err)
    # a test index the caller got wrong is reported, not read
    bad = index.copy()
    bad[2] = 2
    err, counts = device_vsd(v, f, gt, est, test, bad, d)
    assert np.isnan(err[2]).all() and (counts[2] == -1).all()
    keep = [0, 1, 3, 4]
    assert np.array_equal(err[keep], want_err[keep]) and np.array_equal(counts[keep], want_counts[keep])


def test_argument_checks():
    import torch
    from betapose_amd import _lib
    L = _lib.lib()
    v, f = rc.box()
    d_model, d_faces = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    d_pose = torch.zeros((2, 12), dtype=torch.float64, device="cuda")
    d_depth = torch.zeros((2, H, W), dtype=torch.float32, device="cuda")
    d_skip = torch.zeros(2, dtype=torch.int32, device="cuda")
    Kf = np.ascontiguousarray(K).reshape(9)
    p = _lib.ptr
    good = [p(d_model), len(v), p(d_faces), len(f), p(d_pose), 2, p(Kf), H, W, 0.0, 0.01, p(d_depth), p(d_skip), None]
    assert L.bp_render_depth(*good) == 0
    for i, val in [(0, None), (2, None), (4, None), (6, None), (11, None), (12, None), (1, 0), (3, -1), (5, 0), (7, 0), (8, 0),
                   (10, 0.0), (10, -1.0)]:
        args = list(good)
        args[i] = val
        assert L.bp_render_depth(*args) < 0, i
        assert L.bp_last_error()
    args = list(good)
    args[7], args[8] = 4096, 4097           # H * W > 2^24: refused before anything is touched
    assert L.bp_render_depth(*args) < 0

    d_test = torch.zeros((1, H, W), dtype=torch.int16, device="cuda")
    d_idx = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_err = torch.zeros((2, 16), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    taus = np.linspace(0.05, 0.5, 17)
    good = [p(d_model), len(v), p(d_faces), len(f), p(d_pose), p(d_pose), 2, p(Kf), p(d_test), 1, H, W, 0.001, p(d_idx), 0.015,
            p(taus), 16, 0.1, 0.0, 0.01, 0, p(d_err), p(d_cnt), None]
    assert L.bp_vsd_errors(*good) == 0
    for i, val in [(0, None), (2, None), (4, None), (5, None), (7, None), (8, None), (13, None), (15, None), (21, None),
                   (22, None), (1, 0), (3, 0), (6, 0), (9, 0), (10, 0), (11, -3), (12, 0.0), (16, 17), (16, 0), (17, 0.0),
                   (19, 0.0), (20, -1)]:
        args = list(good)
        args[i] = val
        assert L.bp_vsd_errors(*args) < 0, i
    torch.cuda.synchronize()
