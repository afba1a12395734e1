"""bp_pose_errors_sym (csrc/pose_metrics_sym.hip): the BOP errors MSSD and MSPD of many pose pairs over a symmetry set in
one call, f64, against the host numpy definitions (metrics.mssd_err / mspd_err) at the edges of the kernel's tiles
(64-lane waves, 256 symmetries per block, 512 vertices per LDS tile, vertex slices over grid.z), the position of the
winning symmetry and vertex, analytic cases on a large lattice, the `want` mask, run-to-run determinism, argument checks,
evaluate_results(symmetries=...) on the device and the harness's --bop_metrics."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import helpers  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
HALF_TURN_Z = [-1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]
IDENTITY = np.eye(4)[None, :3, :]
FILL = -1.0


def rand_rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def linemod_poses(rng, P):
    """(gt, est) [P, 4, 4]: LineMod-like placements (z 0.6 .. 1.2 m), estimates a few degrees / centimetres off."""
    gt = np.tile(np.eye(4), (P, 1, 1))
    est = gt.copy()
    for p in range(P):
        gt[p, :3, :3] = rand_rot(rng)
        gt[p, :3, 3] = [rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)]
        a = rng.normal(size=3) * 0.05
        th = np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / th
        est[p, :3, :3] = gt[p, :3, :3] @ (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)
        est[p, :3, 3] = gt[p, :3, 3] + rng.normal(size=3) * 0.01
    return gt, est


def random_syms(rng, S):
    """[S, 4, 4]: the identity, then random proper rotations with centimetre translations."""
    s = np.tile(np.eye(4), (S, 1, 1))
    for k in range(1, S):
        s[k, :3, :3] = rand_rot(rng)
        s[k, :3, 3] = rng.normal(size=3) * 0.01
    return s


def device_errors(model, gt, est, syms, cam=CAM, want=3, stream=None):
    import torch
    from betapose_amd import _lib
    syms = np.asarray(syms, dtype=np.float64)
    d_model = torch.from_numpy(np.ascontiguousarray(model, np.float64)).cuda()
    d_gt = torch.from_numpy(np.ascontiguousarray(gt[:, :3, :4].reshape(-1, 12))).cuda()
    d_est = torch.from_numpy(np.ascontiguousarray(est[:, :3, :4].reshape(-1, 12))).cuda()
    d_sym = torch.from_numpy(np.ascontiguousarray(syms[:, :3, :4].reshape(-1, 12))).cuda()
    d_out = torch.full((len(gt), 2), FILL, dtype=torch.float64, device="cuda")
    K = np.ascontiguousarray(cam, np.float64).reshape(9) if cam is not None else None
    s = stream if stream is not None else torch.cuda.current_stream()
    _lib.check(_lib.lib().bp_pose_errors_sym(_lib.ptr(d_model), len(model), _lib.ptr(d_gt), _lib.ptr(d_est), len(gt),
                                             _lib.ptr(d_sym), len(syms), _lib.ptr(K), want, _lib.ptr(d_out),
                                             s.cuda_stream))
    return d_out.cpu().numpy()


def host_errors(model, gt, est, syms, cam=CAM):
    from betapose_amd import metrics
    return np.stack(metrics.pose_errors_sym(gt, est, model, cam, syms), axis=1)


# n at S = 3, P = 3 (wave and LDS-tile edges: 64, 512, 1024; 4099 = nine tiles, split over grid.z); S at n = 257, P = 3
# (wave, block and two-block edges, 630 = discrete x continuous); P at n = 1025, S = 65.  P * S * n <= 2.5e6 each.
CASES = ([(n, 3, 3) for n in (1, 2, 3, 4, 5, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4099)]
         + [(257, S, 3) for S in (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 630)]
         + [(1025, 65, P) for P in (1, 37)])


@pytest.mark.parametrize("n,S,P", CASES)
def test_match_numpy(cuda, n, S, P):
    rng = np.random.default_rng(100000 * n + 100 * S + P)
    model = rng.normal(size=(n, 3)) * [0.05, 0.04, 0.03]
    gt, est = linemod_poses(rng, P)
    syms = random_syms(rng, S)
    dev = device_errors(model, gt, est, syms)
    ref = host_errors(model, gt, est, syms)
    e3, e2 = np.abs(dev[:, 0] - ref[:, 0]).max(), np.abs(dev[:, 1] - ref[:, 1]).max()
    print("n %d S %d P %d: |MSSD dev - host| %.3e m, |MSPD dev - host| %.3e px" % (n, S, P, e3, e2))
    assert e3 < 1e-12, e3
    assert e2 < 1e-9, e2


@pytest.mark.parametrize("n", [1, 65, 1025, 4099])
def test_identity_set_bounds_add_and_2d(cuda, n):
    """With Sym = [I] the two errors are plain maxima over the vertices: never below bp_pose_errors' means."""
    import torch
    from betapose_amd import _lib
    rng = np.random.default_rng(n)
    model = rng.normal(size=(n, 3)) * [0.05, 0.04, 0.03]
    gt, est = linemod_poses(rng, 5)
    dev = device_errors(model, gt, est, IDENTITY)
    d_model = torch.from_numpy(model).cuda()
    d_gt = torch.from_numpy(np.ascontiguousarray(gt[:, :3, :4].reshape(-1, 12))).cuda()
    d_est = torch.from_numpy(np.ascontiguousarray(est[:, :3, :4].reshape(-1, 12))).cuda()
    d_out = torch.zeros((5, 3), dtype=torch.float64, device="cuda")
    K = np.ascontiguousarray(CAM).reshape(9)
    _lib.check(_lib.lib().bp_pose_errors(_lib.ptr(d_model), n, _lib.ptr(d_gt), _lib.ptr(d_est), 5, _lib.ptr(K), 5,
                                         _lib.ptr(d_out), torch.cuda.current_stream().cuda_stream))
    mean = d_out.cpu().numpy()
    # a mean of n values can exceed their maximum by rounding only: n ulp of the value is far below these margins
    assert (dev[:, 0] >= mean[:, 0] - 1e-15).all()
    assert (dev[:, 1] >= mean[:, 2] - 1e-11).all()
    if n == 1:
        assert np.abs(dev[:, 0] - mean[:, 0]).max() < 1e-15 and np.abs(dev[:, 1] - mean[:, 2]).max() < 1e-11


@pytest.mark.parametrize("k", [0, 63, 64, 255, 256])
def test_winning_symmetry_position(cuda, k):
    """est = gt o S_k for one k of 257 random symmetries: only S_k explains the estimate."""
    rng = np.random.default_rng(31)
    n, S = 1025, 257
    model = rng.normal(size=(n, 3)) * [0.05, 0.04, 0.03]
    syms = random_syms(rng, S)
    gt, _ = linemod_poses(rng, 3)
    est = gt @ syms[k]
    dev = device_errors(model, gt, est, syms)
    assert dev[:, 0].max() <= 1e-12 and dev[:, 1].max() <= 1e-9
    others = np.delete(syms, k, axis=0)
    assert device_errors(model, gt, est, others)[:, 0].min() > 1e-3         # ... and no other one does


@pytest.mark.parametrize("idx", [0, 511, 512, 1023, 1024])
def test_farthest_vertex_position(cuda, idx):
    """One vertex ten times as far out as the others, at a tile's first or last slot, decides the result.  The
    estimate is the ground truth turned by 0.05 rad about an axis at right angles to that vertex, and every symmetry
    but the identity turns by 0.5 .. 1 rad about such an axis: under the identity the far vertex moves by
    2 sin(0.025) |x| = 35 mm and no other vertex (|x| < 0.25 m) by more than 13 mm; under any other symmetry the far
    vertex is at least 2 sin(0.225) |x| = 0.31 m off.  So the result is the far vertex's distance under the identity."""
    rng = np.random.default_rng(32)
    n, S = 1025, 257
    model = rng.normal(size=(n, 3)) * [0.05, 0.04, 0.03]
    assert np.linalg.norm(model, axis=1).max() < 0.25
    x = model[idx] = 10.0 * np.array([0.05, -0.04, 0.03])

    def turn_across_x(th):
        a = np.cross(x, rng.normal(size=3))
        a /= np.linalg.norm(a)
        A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        T = np.eye(4)
        T[:3, :3] = np.eye(3) + np.sin(th) * A + (1 - np.cos(th)) * A @ A
        return T
    syms = np.stack([np.eye(4)] + [turn_across_x(rng.uniform(0.5, 1.0)) for _ in range(S - 1)])
    gt, _ = linemod_poses(rng, 3)
    est = np.stack([g @ turn_across_x(0.05) for g in gt])
    dev = device_errors(model, gt, est, syms)
    for p in range(3):
        d_far = np.linalg.norm(est[p, :3, :3] @ x + est[p, :3, 3] - (gt[p, :3, :3] @ x + gt[p, :3, 3]))
        assert abs(d_far - 2 * np.sin(0.025) * np.linalg.norm(x)) < 1e-12
        assert abs(dev[p, 0] - d_far) < 1e-12
    ref = host_errors(model, gt, est, syms)
    assert np.abs(dev[:, 0] - ref[:, 0]).max() < 1e-12 and np.abs(dev[:, 1] - ref[:, 1]).max() < 1e-9


def lattice(h=1e-3, m=147):
    """m x m square lattice of spacing h in the z = 0 plane, centred on the z axis (21 609 points)."""
    c = (np.arange(m) - (m - 1) / 2) * h
    x, y = np.meshgrid(c, c, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(m * m)], axis=1)


def rz44(phi):
    T = np.eye(4)
    c, s = np.cos(phi), np.sin(phi)
    T[:2, :2] = [[c, -s], [s, c]]
    return T


def test_lattice_quarter_turn(cuda):
    rng = np.random.default_rng(7)
    model = lattice()
    assert len(model) == 21609
    gt, _ = linemod_poses(rng, 4)
    q = np.eye(4)
    q[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    c4 = np.stack([np.linalg.matrix_power(q, i) for i in range(4)])
    est = gt @ q
    dev = device_errors(model, gt, est, c4)
    assert dev[:, 0].max() <= 1e-12 and dev[:, 1].max() <= 1e-9
    dev = device_errors(model, gt, est, IDENTITY)
    assert np.abs(dev[:, 0] - np.sqrt(2.0) * np.linalg.norm(model[:, :2], axis=1).max()).max() < 1e-12


def test_half_turn_and_surface_of_revolution(cuda):
    from betapose_amd import metrics
    rng = np.random.default_rng(8)
    n = 21609
    gt, _ = linemod_poses(rng, 4)
    # a half-turn symmetric point set, the estimate turned half-way
    half = rng.normal(size=(n // 2, 3)) * [0.05, 0.04, 0.03]
    model = np.concatenate([half, half * [-1, -1, 1], [[0.0, 0.0, 0.01]]])
    assert len(model) == n
    est = gt @ np.diag([-1.0, -1.0, 1.0, 1.0])
    with_turn = metrics.symmetry_transforms({"symmetries_discrete": [HALF_TURN_Z]})
    dev = device_errors(model, gt, est, with_turn)
    assert dev[:, 0].max() <= 1e-12 and dev[:, 1].max() <= 1e-9
    assert device_errors(model, gt, est, IDENTITY)[:, 0].min() > 1e-2
    # points on circles about z under the 315-step continuous symmetry: 2 r_max sin(delta / 2)
    r = rng.uniform(0.005, 0.05, size=n)
    r[12345] = r_max = 0.05
    a = rng.uniform(0, 2 * np.pi, size=n)
    model = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-0.03, 0.03, size=n)], axis=1)
    cont = metrics.symmetry_transforms({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})
    step = 2 * np.pi / len(cont)
    phis = np.array([0.004, 1.0, -0.77, step * 40.5])
    est = np.stack([g @ rz44(phi) for g, phi in zip(gt, phis)])
    delta = np.abs(phis - step * np.round(phis / step))
    dev = device_errors(model, gt, est, cont, want=1)
    assert np.abs(dev[:, 0] - 2 * r_max * np.sin(delta / 2)).max() < 1e-12


def test_want_mask(cuda):
    rng = np.random.default_rng(9)
    model = rng.normal(size=(700, 3)) * [0.05, 0.04, 0.03]
    gt, est = linemod_poses(rng, 4)
    syms = random_syms(rng, 5)
    both = device_errors(model, gt, est, syms)
    only3 = device_errors(model, gt, est, syms, want=1)
    only2 = device_errors(model, gt, est, syms, want=2)
    assert (only3[:, 1] == FILL).all() and (only2[:, 0] == FILL).all()
    assert np.array_equal(only3[:, 0], both[:, 0]) and np.array_equal(only2[:, 1], both[:, 1])
    no_k = device_errors(model, gt, est, syms, cam=None, want=1)           # K = NULL is accepted without MSPD
    assert np.array_equal(no_k, only3)


def test_bit_identical_across_calls_and_streams(cuda):
    import torch
    rng = np.random.default_rng(11)
    model = rng.normal(size=(4099, 3)) * 0.05
    gt, est = linemod_poses(rng, 1500)
    syms = random_syms(rng, 65)
    a = device_errors(model, gt, est, syms)
    b = device_errors(model, gt, est, syms)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c = device_errors(model, gt, est, syms, stream=s1)
    d = device_errors(model, gt, est, syms, stream=s2)
    assert np.isfinite(a).all() and (a > 0).all()
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert np.array_equal(a.view(np.int64), c.view(np.int64))
    assert np.array_equal(a.view(np.int64), d.view(np.int64))


def test_bad_arguments(cuda):
    """Every rejected call fails in the argument checks, before any launch: the output buffer keeps its fill."""
    import torch
    from betapose_amd import _lib
    L = _lib.lib()
    m = torch.zeros(10, 3, dtype=torch.float64, device="cuda")
    g = torch.zeros(2, 12, dtype=torch.float64, device="cuda")
    g[:, 0] = g[:, 5] = g[:, 10] = 1.0
    g[:, 11] = 1.0
    sy = torch.zeros(3, 12, dtype=torch.float64, device="cuda")
    sy[:, 0] = sy[:, 5] = sy[:, 10] = 1.0
    out = torch.full((2, 2), FILL, dtype=torch.float64, device="cuda")
    K = np.ascontiguousarray(CAM).reshape(9)
    mp, gp, sp, op, kp = m.data_ptr(), g.data_ptr(), sy.data_ptr(), out.data_ptr(), K.ctypes.data
    cases = [((mp, 0, gp, gp, 2, sp, 3, kp, 3, op), "positive"), ((mp, -3, gp, gp, 2, sp, 3, kp, 3, op), "positive"),
             ((mp, 10, gp, gp, 0, sp, 3, kp, 3, op), "positive"), ((mp, 10, gp, gp, -1, sp, 3, kp, 3, op), "positive"),
             ((mp, 10, gp, gp, 2, sp, 0, kp, 3, op), "positive"), ((mp, 10, gp, gp, 2, sp, -2, kp, 3, op), "positive"),
             ((None, 10, gp, gp, 2, sp, 3, kp, 3, op), "null"), ((mp, 10, None, gp, 2, sp, 3, kp, 3, op), "null"),
             ((mp, 10, gp, None, 2, sp, 3, kp, 3, op), "null"), ((mp, 10, gp, gp, 2, None, 3, kp, 3, op), "null"),
             ((mp, 10, gp, gp, 2, sp, 3, kp, 3, None), "null"),
             ((mp, 10, gp, gp, 2, sp, 3, None, 2, op), "K is required"), ((mp, 10, gp, gp, 2, sp, 3, None, 3, op), "K is required"),
             ((mp, 10, gp, gp, 2, sp, 3, kp, 0, op), "want"), ((mp, 10, gp, gp, 2, sp, 3, kp, 4, op), "want"),
             ((mp, 10, gp, gp, 2, sp, 3, kp, -1, op), "want")]
    for args, text in cases:
        assert L.bp_pose_errors_sym(*args, None) < 0, args
        assert text in L.bp_last_error().decode(), (args, L.bp_last_error())
    assert (out.cpu().numpy() == FILL).all()
    assert L.bp_pose_errors_sym(mp, 10, gp, gp, 2, sp, 3, None, 1, op, None) == 0    # K may be NULL without MSPD
    got = out.cpu().numpy()
    assert (got[:, 0] == 0.0).all() and (got[:, 1] == FILL).all()


def test_evaluate_results_device_equals_host(cuda, tmp_path):
    import evaluate
    from betapose_amd import metrics, synth
    rng = np.random.default_rng(21)
    half = rng.normal(size=(600, 3)) * [40.0, 30.0, 20.0]
    model_mm = np.concatenate([half, half * [-1, -1, 1]])     # symmetric under a half turn about z
    gt_by, final_result = {}, []
    for nr in range(40):
        g, e = linemod_poses(rng, 1)
        g, e = g[0], e[0]
        if nr % 4 == 1:
            e = e.copy()
            e[:3, :3] = e[:3, :3] @ np.diag([-1.0, -1.0, 1.0])
        box = [100.0 + 2 * nr, 90.0, 120.0, 100.0]
        gt_by[nr] = [(1, g[:3, :3], g[:3, 3] * 1000.0, box)]
        off = 80.0 if nr % 7 == 3 else 3.0
        final_result.append({"imgname": "%04d.png" % nr, "cam_R": e[:3, :3], "cam_t": e[:3, 3:4],
                             "result": [{"bbox": [box[0] + off, box[1], box[0] + box[2] + off, box[1] + box[3]]}]})
    synth.write_sixd_tree(str(tmp_path), 1, gt_by, {1: model_mm}, {1: half[:50]}, {1: 100.0},
                          symmetries={1: {"symmetries_discrete": [HALF_TURN_Z]}})
    frames, model, _, diameter, cam = evaluate.load_sixd_gt(str(tmp_path), 1)
    syms = metrics.load_symmetries(str(tmp_path), 1)
    assert syms.shape == (2, 3, 4)
    # no error within 1e-9 of a threshold
    gts = np.stack([frames[nr][0]["pose"] for nr in range(40)])
    ests = np.stack([np.vstack((np.hstack((f["cam_R"], f["cam_t"])), [0, 0, 0, 1])) for f in final_result])
    mssd, mspd = metrics.pose_errors_sym(gts, ests, model, cam, syms)
    for k in range(1, 11):
        assert np.abs(mssd - 0.05 * k * diameter / 1000.0).min() > 1e-9
        assert np.abs(mspd - 5.0 * k).min() > 1e-9
    host = metrics.evaluate_results(final_result, frames, model, cam, diameter, symmetries=syms)
    dev = metrics.evaluate_results(final_result, frames, model, cam, diameter, symmetries=syms, device=cuda)
    assert set(host) == set(dev) and {"ar_mssd", "ar_mspd", "mean_mssd_err_mm", "mean_mspd_err_px"} <= set(host)
    for k in ("ar_mssd", "ar_mspd", "n"):
        assert host[k] == dev[k], k
    for k in ("mean_mssd_err_mm", "mean_mspd_err_px"):
        assert abs(host[k] - dev[k]) < 1e-9, k
    plain = metrics.evaluate_results(final_result, frames, model, cam, diameter, symmetries=IDENTITY, device=cuda)
    assert 0 < plain["ar_mssd"] < host["ar_mssd"]               # the flipped frames count


METRIC_LINE = re.compile(r"^(Mean add accuracy|Mean add-s accuracy|2d reprojection accuracy|Mean IoU|Mean mssd recall|"
                         r"Mean mspd recall) for seq (\d+) is: (\S+)$", re.M)


def test_harness_bop_metrics(tmp_path, cuda):
    """evaluate.py on frame files + a SIXD tree whose ground truth is the pipeline's own poses: frame 0 as estimated,
    frame 1 turned half-way about the (half-turn symmetric) model's z axis, frame 2 moved 30 cm; the tree declares the
    half turn.  --bop_metrics adds the two recall lines after the three of before, with the host metric's values."""
    from PIL import Image
    from betapose_amd import metrics, synth
    from betapose_amd.darknet import Darknet
    from betapose_amd.kpd import FastPoseHIP
    from betapose_amd.pipeline import FramePipeline, finish_record
    from betapose_amd.weights import fastpose_stream_from_state_dict

    obj_id = 1
    frames = helpers.frames(3)
    indir = tmp_path / "rgb"
    indir.mkdir()
    for i, fr in enumerate(frames):
        Image.fromarray(fr[:, :, ::-1].copy()).save(indir / ("%04d.png" % i))
    kp_mm = np.round(synth.synth_kp3d(50) * 1000.0, 6)
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416).load_stream(helpers.yolo_stream()).cuda()
    pose = FastPoseHIP.from_stream(fastpose_stream_from_state_dict(helpers.kpd_state_dict(), 50), n_classes=50).cuda()
    pipe = FramePipeline(det, pose, 480, 640, batch=1, confidence=0.01)
    gt, boxes = {}, {}
    for i, fr in enumerate(frames):
        out = finish_record(pipe.run(fr)[0], "%04d.png" % i, kp_mm / 1000.0, synth.CAM_K, 50)
        assert out["boxes"] is not None and len(out["result"]) == 1
        R, t = np.asarray(out["cam_R"]), np.asarray(out["cam_t"]).reshape(3)
        if i == 1:
            R = R @ np.diag([-1.0, -1.0, 1.0])
        if i == 2:
            t = t + [0.3, 0.0, 0.0]
        x1, y1, x2, y2 = [float(v) for v in out["result"][0]["bbox"]]
        boxes["%04d.png" % i] = [x1, y1, x2, y2]
        gt[i] = [(obj_id, R, t * 1000.0, [x1, y1, x2 - x1, y2 - y1])]
    del pipe, det, pose
    rng = np.random.default_rng(0)
    half = np.round(rng.normal(size=(400, 3)) * 30.0, 6)
    synth.write_sixd_tree(str(tmp_path / "sixd"), obj_id, gt, {obj_id: np.concatenate([half, half * [-1, -1, 1]])},
                          {obj_id: kp_mm}, {obj_id: 100.0}, symmetries={obj_id: {"symmetries_discrete": [HALF_TURN_Z]}})

    def run(extra, name):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--indir", str(indir), "--outdir", str(out),
                            "--sixd_base", str(tmp_path / "sixd"), "--synth_weights", "--fused", "--obj_id", str(obj_id)]
                           + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout, json.loads(open(out / "Betapose-results.json").read())

    plain, _ = run([], "plain")
    assert [m[0] for m in METRIC_LINE.findall(plain)] == ["Mean add accuracy", "2d reprojection accuracy", "Mean IoU"]
    assert "mssd" not in plain and "mspd" not in plain
    bop, res = run(["--bop_metrics"], "bop")
    lines = METRIC_LINE.findall(bop)
    assert [m[0] for m in lines] == ["Mean add accuracy", "2d reprojection accuracy", "Mean IoU", "Mean mssd recall",
                                     "Mean mspd recall"]
    assert lines[:3] == METRIC_LINE.findall(plain)

    import evaluate
    frames_gt, model, _, diameter, cam = evaluate.load_sixd_gt(str(tmp_path / "sixd"), obj_id)
    final_result = [{"imgname": r_["image_id"], "cam_R": np.array(r_["cam_R"]).reshape(3, 3),
                     "cam_t": np.array(r_["cam_t"]).reshape(3, 1), "result": [{"bbox": boxes[r_["image_id"]]}]}
                    for r_ in res]
    host = metrics.evaluate_results(final_result, frames_gt, model, cam, diameter,
                                    symmetries=metrics.load_symmetries(str(tmp_path / "sixd"), obj_id))
    printed = dict((m[0], m[2]) for m in lines)
    assert printed["Mean mssd recall"] == "%.3f" % host["ar_mssd"]
    assert printed["Mean mspd recall"] == "%.3f" % host["ar_mspd"]
    # frames 0 and 1 are exact under the half turn, frame 2 misses every threshold (300 mm against at most 50 mm)
    assert printed["Mean mssd recall"] == "0.667"
