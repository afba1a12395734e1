"""Device RANSAC PnP (csrc/pnp_ransac.hip) against the host solver ``bp_solve_pnp_ransac``, problem by problem: the
device result must be the result of the host's sequential loop -- inlier masks and statuses equal, R and t within the
bars tests/test_gpu_pose_tail.py uses for the same solver against the same host code (1e-9 on noise-free / Gaussian
inputs, 1e-6 on the rest, t relative to the model scale; a problem beyond the bar must be one the host solver itself
moves on when its input changes by one ulp, and such problems must stay rare).

Precondition (asserted for every problem, none dropped): the two solvers agree only to rounding, so a point whose
reprojection error sits on the threshold could flip.  ``_restated_loop`` restates the host's trial loop in numpy over
``ops.solve_pnp`` / ``ops.pnp_ransac_samples`` / ``ops.pnp_ransac_trials_needed``; it must reproduce the host's mask,
and no point of any executed trial may lie within 1e-4 px of the threshold."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation as Rot

pytestmark = pytest.mark.gpu

import helpers  # noqa: E402
from betapose_amd import _lib, ops, synth  # noqa: E402
from betapose_amd.synth import CAM_K, synth_kp3d  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP3D = synth_kp3d(50)
MARGIN = 1e-4
FRAME_DIAGONAL = 800.0     # px: 640 x 480 frames; see test_pipeline_with_ransac


def _project(P, R, t):
    uv = (P @ R.T + t) @ CAM_K.T
    return uv[:, :2] / uv[:, 2:]


def _poses(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        R = Rot.from_rotvec(rng.normal(0, 0.9, 3)).as_matrix()
        t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 1.5)])
        yield R, t, rng


def _restated_loop(P, U, err, trials, conf):
    """The host's trial loop restated: returns (status, mask, executed trials, smallest |error - threshold| seen)."""
    n = len(P)
    if n < 6:
        return -1, np.zeros(n, bool), 0, np.inf
    if n == 6:
        return 0, np.ones(n, bool), 0, np.inf
    idx = ops.pnp_ransac_samples(n, trials)
    need = ops.pnp_ransac_trials_needed(n, conf)
    best, best_cnt, limit, it, margin = np.zeros(n, bool), 0, trials, 0, np.inf
    while it < limit:
        try:
            R, t = ops.solve_pnp(P[idx[it]], U[idx[it]], CAM_K)
        except _lib.BetaposeHipError:
            it += 1
            continue
        e = np.linalg.norm(_project(P, R, t[:, 0]) - U, axis=1)
        margin = min(margin, np.abs(e - err).min())
        cur = e <= err
        if cur.sum() > best_cnt:
            best_cnt, best = int(cur.sum()), cur
            if need[best_cnt] < limit:
                limit = max(it + 1, int(need[best_cnt]))
        it += 1
    return (0 if best_cnt >= 6 else -2), (best if best_cnt >= 6 else np.zeros(n, bool)), limit, margin


def _host(P, U, err, trials, conf):
    """(status, R, t, mask) of the host solver; the status of a failure is told apart by the restated loop."""
    try:
        R, t, inl = ops.solve_pnp_ransac(P, U, CAM_K, err, trials, conf)
        return 0, R, t[:, 0], inl
    except _lib.BetaposeHipError:
        return -2, None, None, np.zeros(len(P), bool)


def _one_ulp_sensitivity(p3, p2, scale):
    R0, t0 = ops.solve_pnp(p3, p2, CAM_K)
    s = 0.0
    for d in (np.inf, -np.inf):
        for a, b in ((np.nextafter(p3, d), p2), (p3, np.nextafter(p2, d))):
            R, t = ops.solve_pnp(a, b, CAM_K)
            s = max(s, np.abs(R - R0).max(), np.abs(t - t0).max() / scale)
    return s


def _family(n, scale, seed, poses=3):
    """Planted-outlier problems of n points: outlier share 0 / 20 / 40 / 60 %, inlier noise sigma 0 / 0.5 px; returns
    (P3 [p][n][3], P2 [p][n][2], tolerance per problem)."""
    P = KP3D[:n] * 3.0 * scale
    P3, P2, tol = [], [], []
    for share in (0.0, 0.2, 0.4, 0.6):
        for sigma in (0.0, 0.5):
            for R, t, rng in _poses(poses, seed + int(share * 10) * 7 + int(sigma * 2)):
                uv = _project(P, R, t * scale) + rng.normal(0, sigma, (n, 2))
                nb = int(round(share * n))
                bad = rng.choice(n, nb, replace=False)
                uv[bad] += rng.uniform(30, 120, (nb, 2)) * rng.choice([-1, 1], (nb, 2))
                P3.append(P)
                P2.append(uv)
                tol.append(1e-9 if share == 0 else 1e-6)
    return np.array(P3), np.array(P2), np.array(tol)


def _check(P3, P2, tol, scale=1.0, shared=False, err=12.0, trials=100, conf=0.99, want_trials=None):
    """One device launch over all problems against the host, problem by problem."""
    Rt, st, inl = ops.solve_pnp_ransac_batch(P3[0] if shared else P3, P2, CAM_K, err, trials, conf)
    Rt, st, inl = Rt.cpu().numpy(), st.cpu().numpy(), inl.cpu().numpy()
    beyond, executed = 0, []
    for p in range(len(P2)):
        hst, hR, ht, hinl = _host(P3[p], P2[p], err, trials, conf)
        rst, rmask, ran, margin = _restated_loop(P3[p], P2[p], err, trials, conf)
        executed.append(ran)
        print("problem %d: host status %d inliers %d, device status %d inliers %d, trials run %d, margin %.3g px" % (
            p, hst, hinl.sum(), st[p], inl[p].sum(), ran, margin))
        assert margin >= MARGIN, (p, margin)                                        # the precondition
        assert (rst < 0) == (hst < 0) and (hst < 0 or np.array_equal(rmask, hinl)), p   # ... and the restatement is the host's
        assert (st[p] < 0) == (hst < 0), (p, st[p], hst)
        if hst < 0:
            assert st[p] == rst and np.isnan(Rt[p]).all() and not inl[p].any(), p
            continue
        assert st[p] == 0 and np.array_equal(inl[p], hinl), (p, inl[p], hinl)
        d = max(np.abs(Rt[p][:, :3] - hR).max(), np.abs(Rt[p][:, 3] - ht).max() / scale)
        if d > tol[p]:
            sens = _one_ulp_sensitivity(np.ascontiguousarray(P3[p][hinl]), np.ascontiguousarray(P2[p][hinl]), scale)
            assert d <= 10 * sens, (p, d, sens)
            beyond += 1
    assert beyond <= max(1, len(P2) // 20), (beyond, len(P2))
    if want_trials is not None:
        want_trials(np.array(executed))
    return st, inl


@pytest.mark.parametrize("scale", [1.0, 1000.0])
@pytest.mark.parametrize("n", [50, 20, 10, 7, 6])
def test_batch_planted_outlier_families(cuda, n, scale):
    P3, P2, tol = _family(n, scale, 100 + n)
    st, inl = _check(P3, P2, tol, scale)
    assert (st[:6] == 0).all() and inl[:6].all()           # the outlier-free problems keep every point
    st2, _ = _check(P3, P2, tol, scale, shared=True)        # one model for every problem
    np.testing.assert_array_equal(st, st2)


def test_early_stop_is_replayed(cuda):
    P3, P2, tol = _family(50, 1.0, 900)

    def stops_early(ran):
        assert (ran[:6] <= 10).all(), ran                   # no outliers: the host stops after a handful of trials
        assert (ran[18:] == 100).all(), ran                 # 60 % outliers: every trial runs
    _check(P3, P2, tol, want_trials=stops_early)
    def one(ran):
        assert (ran == 1).all(), ran
    _check(P3, P2, tol, trials=1, want_trials=one)
    for conf in (0.5, 0.999):
        _check(P3, P2, tol, conf=conf)
    P3, P2, tol = _family(20, 1.0, 901)
    _check(P3, P2, tol, trials=300, conf=0.999)             # more trials than one hypothesis launch carries samples for


def test_statuses_and_bad_arguments(cuda):
    rng = np.random.default_rng(5)
    P3, P2, tol = _family(20, 1.0, 78)
    _check(P3, P2, tol)
    Rt, st, inl = ops.solve_pnp_ransac_batch(P3[:, :5], P2[:, :5], CAM_K)                # n = 5
    assert (st.cpu().numpy() == -1).all() and torch.isnan(Rt).all() and not inl.any()
    rand2d = rng.uniform(50, 450, (8, 20, 2))                                            # no projection of anything
    mixed3, mixed2 = np.concatenate([P3[:6], P3[:8], P3[6:12]]), np.concatenate([P2[:6], rand2d, P2[6:12]])
    Rt, st, inl = ops.solve_pnp_ransac_batch(mixed3, mixed2, CAM_K, 0.5)
    Rt, st, inl = Rt.cpu().numpy(), st.cpu().numpy(), inl.cpu().numpy()
    assert (st[6:14] == -2).all() and np.isnan(Rt[6:14]).all() and not inl[6:14].any()
    for p in range(8):
        assert _host(mixed3[6 + p], mixed2[6 + p], 0.5, 100, 0.99)[0] == -2
    alone = ops.solve_pnp_ransac_batch(np.concatenate([P3[:6], P3[6:12]]), np.concatenate([P2[:6], P2[6:12]]), CAM_K, 0.5)
    keep = np.r_[0:6, 14:20]                                                             # the good ones are untouched
    np.testing.assert_array_equal(Rt[keep].view(np.int64), alone[0].cpu().numpy().view(np.int64))
    np.testing.assert_array_equal(st[keep], alone[1].cpu().numpy())
    np.testing.assert_array_equal(inl[keep], alone[2].cpu().numpy())
    assert (st[:3] == 0).all()                                                           # noise-free problems solve at 0.5 px
    p3, p2 = torch.from_numpy(P3[0]).cuda(), torch.from_numpy(P2).cuda()
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    for kw in (dict(workspace=small), dict(iterations=0), dict(iterations=-3), dict(confidence=0.0), dict(confidence=1.0),
               dict(reprojection_error=0.0)):
        with pytest.raises(_lib.BetaposeHipError):
            ops.solve_pnp_ransac_batch(p3, p2, CAM_K, **kw)
    with pytest.raises(_lib.BetaposeHipError):
        ops.solve_pnp_ransac_batch(np.zeros((65, 3)), np.zeros((2, 65, 2)), CAM_K)       # n > 64


def test_deterministic_across_calls_and_streams(cuda):
    P3, P2, _ = _family(50, 1.0, 333)
    p3, p2 = torch.from_numpy(P3).cuda(), torch.from_numpy(P2).cuda()
    a = ops.solve_pnp_ransac_batch(p3, p2, CAM_K)
    b = ops.solve_pnp_ransac_batch(p3, p2, CAM_K)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c = ops.solve_pnp_ransac_batch(p3, p2, CAM_K)
    with torch.cuda.stream(s2):
        d = ops.solve_pnp_ransac_batch(p3, p2, CAM_K)
    torch.cuda.synchronize()
    for other in (b, c, d):
        np.testing.assert_array_equal(a[0].cpu().numpy().view(np.int64), other[0].cpu().numpy().view(np.int64))
        assert torch.equal(a[1], other[1]) and torch.equal(a[2], other[2])
    assert (a[1] == 0).sum() >= 18


# ---------------------------------------------------------------- the tail on records
def _record(rng, R, t, det=True, n_out=0):
    """A frame record whose 50 arg-max pixels come from projecting KP3D with (R, t) into a crop window (quantised to the
    heat-map grid, as a key-point net would emit them), ``n_out`` of them moved 8 .. 24 cells away."""
    rec = np.zeros(316, np.float32)
    rec[0] = np.array([5 if det else -1], np.int32).view(np.float32)[0]
    uv = _project(KP3D, R, t)
    c = uv.mean(axis=0)
    ul = (c - np.array([110.0, 130.0])).astype(np.float32)
    br = (c + np.array([90.0, 120.0])).astype(np.float32)
    rec[1:5] = [10, 20, 30, 40]
    rec[5] = 0.875
    rec[8:10], rec[10:12] = ul, br
    rec[12:16] = [ul[0] + 5, ul[1] + 7, br[0] - 4, br[1] - 6]
    sx, sy = (br[0] - ul[0]) * 1.25, br[1] - ul[1]
    lenH = max(sx, sy)
    dx = max((lenH * 0.8 - 1) / 2 - ((br[0] - 1) - ul[0]) / 2, 0)
    dy = max((lenH - 1) / 2 - ((br[1] - 1) - ul[1]) / 2, 0)
    hx = np.round((uv[:, 0] - ul[0] + dx) * 80 / lenH - 0.2).astype(np.int64)
    hy = np.round((uv[:, 1] - ul[1] + dy) * 80 / lenH - 0.2).astype(np.int64)
    bad = rng.choice(50, n_out, replace=False)
    hx[bad] += rng.integers(8, 25, n_out) * rng.choice([-1, 1], n_out)
    hy[bad] += rng.integers(8, 25, n_out) * rng.choice([-1, 1], n_out)
    hx, hy = np.clip(hx, 0, 63).astype(np.int32), np.clip(hy, 0, 79).astype(np.int32)
    kp = rec[16:].reshape(50, 6)
    kp[:, 0] = (hy * 64 + hx).astype(np.int32).view(np.float32)
    kp[:, 1] = rng.uniform(0.35, 0.95, 50).astype(np.float32)
    kp[:, 2:] = rng.uniform(0, 0.3, (50, 4)).astype(np.float32)
    return rec


def _records():
    recs = []
    for k, (R, t, rng) in enumerate(_poses(6, 11)):
        recs.append(_record(rng, R, t, n_out=(0, 5, 10, 15, 20, 12)[k]))
    rng = np.random.default_rng(3)
    R, t = np.eye(3), np.array([0.01, -0.02, 0.7])
    recs.append(_record(rng, R, t, det=False))                        # no detection
    r = _record(rng, R, t); r[16 + 1::6][:50] = 0.2; recs.append(r)    # dropped by pPose-NMS
    r = _record(rng, R, t)                                             # no consensus: arg-max pixels of nothing
    r[16::6][:50] = rng.integers(0, 80 * 64, 50).astype(np.int32).view(np.float32)
    recs.append(r)
    return np.array(recs)


def _same_dict(a, b, tol, what=""):
    assert a.keys() == b.keys(), (what, a.keys(), b.keys())
    assert a["imgname"] == b["imgname"]
    if a["boxes"] is None:
        assert b["boxes"] is None and a["result"] == [] == b["result"] and a["cam_R"] == [] == b["cam_R"]
        return
    np.testing.assert_array_equal(a["boxes"], b["boxes"])
    np.testing.assert_array_equal(a["scores"], b["scores"])
    assert a["yolo_index"] == b["yolo_index"]
    assert len(a["result"]) == len(b["result"]), what
    for ra, rb in zip(a["result"], b["result"]):
        assert ra.keys() == rb.keys()
        for k in ra:                                                  # bit-identical decode / NMS
            assert ra[k].dtype == rb[k].dtype and ra[k].shape == rb[k].shape, (what, k)
            np.testing.assert_array_equal(ra[k].view(np.int32), rb[k].view(np.int32), err_msg="%s %s" % (what, k))
    if not a["result"]:
        assert a["cam_R"] == [] == b["cam_R"] and a["cam_t"] == [] == b["cam_t"]
        return
    np.testing.assert_array_equal(a["pnp_inliers"], b["pnp_inliers"], err_msg=what)
    d = max(np.abs(a["cam_R"] - b["cam_R"]).max(), np.abs(a["cam_t"] - b["cam_t"]).max())
    assert d <= tol, (what, d)


def _compare_rows(recs, rows, kp3d, left, ransac, tol):
    """Rows of the device RANSAC tail against finish_record(..., ransac=...); returns how many frames got a pose."""
    from betapose_amd.pipeline import finish_pose_record, finish_record
    n_pose = 0
    for i, (rec, row) in enumerate(zip(recs, rows)):
        name = "%04d.png" % i
        assert row[0] in (1, 2) or int(row[1]) == min(50, left)
        try:
            want = finish_record(rec, name, kp3d, CAM_K, left, ransac=ransac)
        except _lib.BetaposeHipError:
            with pytest.raises(_lib.BetaposeHipError):
                finish_pose_record(rec, row, name)
            assert row[0] < 0 and row[15] == 0 and np.isnan(row[2:14]).all()
            continue
        got = finish_pose_record(rec, row, name)
        _same_dict(got, want, tol, "frame %d left %d" % (i, left))
        if want["result"]:
            assert row[0] == 0
            mask = sum(1 << j for j in range(len(want["pnp_inliers"])) if want["pnp_inliers"][j])
            assert row[15] == float(mask) and int(row[15]) == mask              # slot 15 is the host mask
            n_pose += 1
        else:
            assert row[15] == 0
    return n_pose


@pytest.mark.parametrize("left", [50, 10, 6])
def test_pose_from_records_ransac_matches_finish_record(cuda, left):
    recs = _records()
    dev = torch.from_numpy(recs).cuda()
    rows = ops.pose_from_records_ransac(dev, KP3D, CAM_K, left, 12.0, 100, 0.99).cpu().numpy()
    plain = ops.pose_from_records(dev, KP3D, CAM_K, left).cpu().numpy()
    assert rows[6, 0] == 1 and rows[7, 0] == 2
    if left > 6:
        assert rows[8, 0] == -2                                                  # no consensus
    assert _compare_rows(recs, rows, KP3D, left, (12.0, 100, 0.99), 1e-6) >= (6 if left == 6 else 4)
    other = np.r_[1, 14, 16:166]                                                 # every other slot as today
    np.testing.assert_array_equal(rows[:, other].view(np.int64), plain[:, other].view(np.int64))
    np.testing.assert_array_equal(rows[6:8].view(np.int64), plain[6:8].view(np.int64))
    small = torch.empty(64, dtype=torch.uint8, device="cuda")
    out = torch.empty((len(recs), 166), dtype=torch.float64, device="cuda")
    k3 = torch.from_numpy(KP3D).cuda()
    Kc = np.ascontiguousarray(CAM_K, dtype=np.float64)
    rc = _lib.lib().bp_pose_from_records_ransac(dev.data_ptr(), len(recs), k3.data_ptr(), 50, Kc.ctypes.data, left, 12.0, 100, 0.99,
                                                out.data_ptr(), small.data_ptr(), small.numel(), None)
    assert rc != 0                                                               # too small a workspace: refused


# ---------------------------------------------------------------- in the frame pipeline
def _engines(max_batch, mode):
    from betapose_amd.darknet import Darknet
    from betapose_amd.kpd import FastPoseHIP
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416, max_batch=max_batch).load_stream(helpers.yolo_stream()).cuda()
    pose = FastPoseHIP(helpers.kpd_state_dict(), n_classes=50, max_batch=max_batch).cuda()
    det.set_precision(mode)
    pose.set_precision(mode)
    return det, pose


@pytest.mark.parametrize("batch", [1, 28])
def test_pipeline_with_ransac(cuda, batch):
    """The 64 reference frames (bf16x3, graph replay) with the RANSAC tail: rows equal the host tail on the same
    records.  The frames come from random weights, so their key points are no projection of anything and no consensus
    exists at a few pixels; the reprojection error used is the frame diagonal (800 px for 640 x 480), within which every
    key point of a hypothesis that keeps the object in front of the camera is an inlier -- the sampler, the early stop,
    the selection and the refit all run, and a frame reaches status 0 when its best hypothesis does.  Then RANSAC off
    again: rows bit-identical to a pipeline that never had it on."""
    from betapose_amd.pipeline import FramePipeline
    frames64 = synth.synth_frames(64, helpers.FRAME_SEED)
    det, pose = _engines(batch, "bf16x3")
    pipe = FramePipeline(det, pose, 480, 640, batch=batch)
    launches = [np.stack(frames64[i:i + batch]) for i in range(0, 64 - batch + 1, batch)]
    pipe.set_pose_solver(KP3D, CAM_K, 10)
    never = []
    for f in launches:
        pipe.run(f)
        never.append(pipe.poses.cpu().numpy().copy())
    n1 = pipe.kernel_count()
    ransac = (FRAME_DIAGONAL, 100, 0.99)
    with pytest.raises(_lib.BetaposeHipError):
        pipe.set_pose_ransac((12.0, 100, 1.5))
    pipe.set_pose_solver(KP3D, CAM_K, 10, ransac=ransac)
    recs, rows = [], []
    for _ in range(2):                                                           # the second pass replays the graph
        recs, rows = [], []
        for f in launches:
            recs.append(pipe.run(f))
            rows.append(pipe.poses.cpu().numpy().copy())
    assert pipe.kernel_count() == n1 + 2                                         # prepare, hypotheses, select for one launch
    recs, rows = np.concatenate(recs), np.concatenate(rows)
    n_pose = _compare_rows(recs, rows, KP3D, 10, ransac, 1e-6)
    detected = int((rows[:, 0] != 1).sum())
    print("batch %d: %d frames, %d detected, %d reached status 0 with RANSAC at %.0f px" % (batch, len(rows), detected, n_pose,
                                                                                           FRAME_DIAGONAL))
    assert n_pose >= len(rows) / 2
    pipe.set_pose_ransac(None)
    for f, want in zip(launches, never):
        pipe.run(f)
        np.testing.assert_array_equal(pipe.poses.cpu().numpy().view(np.int64), want.view(np.int64))
    assert pipe.kernel_count() == n1


# ---------------------------------------------------------------- harness
def _run(args):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_evaluate_synthetic_pnp_ransac(tmp_path):
    """evaluate.py --synthetic 16 --fused --pnp_ransac: host tail against --device_pnp, as
    test_gpu_pose_tail.py::test_evaluate_synthetic_device_pnp (1e-6).  Synthetic weights: the frame diagonal as the
    reprojection error, see test_pipeline_with_ransac."""
    outs = {}
    for flag in ([], ["--device_pnp"]):
        od = tmp_path / ("dev" if flag else "host")
        outs[bool(flag)] = _run([os.path.join(ROOT, "evaluate.py"), "--synthetic", "16", "--outdir", str(od), "--fused",
                                 "--left_keypoints", "10", "--pnp_ransac", str(FRAME_DIAGONAL)] + flag)
    poses = [re.search(r"(\d+) with a pose", outs[k]).group(1) for k in (False, True)]
    assert poses[0] == poses[1] and int(poses[0]) > 0
    ja, jb = (json.load(open(tmp_path / d / "Betapose-results.json")) for d in ("host", "dev"))
    assert len(ja) == len(jb)
    for x, y in zip(ja, jb):
        assert x["image_id"] == y["image_id"] and x["keypoints"] == y["keypoints"] and x["score"] == y["score"]
        assert np.abs(np.subtract(x["cam_R"], y["cam_R"])).max() <= 1e-6
        assert np.abs(np.subtract(x["cam_t"], y["cam_t"])).max() <= 1e-6
