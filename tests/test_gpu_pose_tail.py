"""Device pose tail (csrc/pose_tail.hip): key-point decode, pPose-NMS at n = 1, --left_keypoints pruning and the PnP on
the GPU, held to the host tail (pipeline.finish_record, ops.solve_pnp) on the same inputs.

Bars: status, key points used, post-NMS key points and scores, proposal score bit-identical; R, t
<= 1e-9 on the noise-free and Gaussian-noise families (t relative to the model scale), <= 1e-6 on outlier-laden inputs
and on key points of random-weight networks, <= 2e-3 on the near-planar ill-conditioned family (test_pnp.py's bar
between two restatements)."""
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
from betapose_amd.ops import solve_pnp, solve_pnp_batch  # noqa: E402
from betapose_amd.synth import CAM_K, synth_kp3d  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP3D = synth_kp3d(50)


def _project(P, R, t):
    Y = P @ R.T + t
    uv = Y @ CAM_K.T
    return uv[:, :2] / uv[:, 2:]


def _poses(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        R = Rot.from_rotvec(rng.normal(0, 0.9, 3)).as_matrix()
        t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 1.5)])
        yield R, t, rng


def _host(P3, P2):
    """ops.solve_pnp per problem -> (R [P,3,3], t [P,3], status [P]) with the host's failures as status -1."""
    Rs, ts, st = [], [], []
    for p3, p2 in zip(P3, P2):
        try:
            R, t = solve_pnp(p3, p2, CAM_K)
            Rs.append(R); ts.append(t[:, 0]); st.append(0)
        except _lib.BetaposeHipError:
            Rs.append(np.full((3, 3), np.nan)); ts.append(np.full(3, np.nan)); st.append(-1)
    return np.array(Rs), np.array(ts), np.array(st)


def _one_ulp_sensitivity(p3, p2, scale):
    """How far the HOST solver itself moves when its input is perturbed by one ulp (2-D or 3-D points, up or down)."""
    R0, t0 = solve_pnp(p3, p2, CAM_K)
    s = 0.0
    for d in (np.inf, -np.inf):
        for a, b in ((np.nextafter(p3, d), p2), (p3, np.nextafter(p2, d))):
            R, t = solve_pnp(a, b, CAM_K)
            s = max(s, np.abs(R - R0).max(), np.abs(t - t0).max() / scale)
    return s


def _check_batch(P3, P2, tol, scale=1.0, shared=False):
    """One launch over all problems against the host solver, problem by problem.  The device agrees with the host to
    ``tol``; a problem beyond it must be one the host solver itself moves on by at least a tenth as much when its input
    changes by one ulp (the 20-step, FLT_EPSILON-terminated minimiser amplifies the last bits of its start), and such
    problems must stay rare."""
    R, t, st = solve_pnp_batch(P3[0] if shared else P3, P2, CAM_K)
    R, t, st = R.cpu().numpy(), t.cpu().numpy()[:, :, 0], st.cpu().numpy()
    P3 = np.broadcast_to(P3[0], (len(P2),) + P3[0].shape) if shared else P3
    hR, ht, hst = _host(P3, P2)
    np.testing.assert_array_equal(st < 0, hst < 0)
    ok = st == 0
    assert np.isnan(R[~ok]).all() and np.isnan(t[~ok]).all()
    d = np.zeros(len(P2))
    d[ok] = np.maximum(np.abs(R[ok] - hR[ok]).reshape(ok.sum(), -1).max(axis=1), np.abs(t[ok] - ht[ok]).max(axis=1) / scale)
    beyond = np.flatnonzero(d > tol)
    for p in beyond:
        sens = _one_ulp_sensitivity(np.ascontiguousarray(P3[p]), P2[p], scale)
        assert d[p] <= 10 * sens, (p, d[p], sens)
    assert len(beyond) <= max(1, len(P2) // 20), (len(beyond), len(P2), d.max())
    return st


@pytest.mark.parametrize("scale", [1.0, 1000.0])
@pytest.mark.parametrize("npts", [50, 10, 8, 6])
def test_batch_noise_free_and_gaussian_families(cuda, scale, npts):
    P = synth_kp3d(50)[:npts] * scale
    P2 = []
    for sigma in (0.0, 0.3, 1.0, 3.0):
        for R, t, rng in _poses(16, 2 + npts):
            P2.append(_project(P, R, t * scale) + rng.normal(0, sigma, (npts, 2)))
    P2 = np.array(P2)
    _check_batch(np.broadcast_to(P, (len(P2),) + P.shape).copy(), P2, 1e-9, scale)
    _check_batch(P[None], P2, 1e-9, scale, shared=True)             # one model for every problem


def test_batch_planar_branch_and_four_points(cuda):
    P = synth_kp3d(50).copy()
    P[:, 2] = 0.01
    P = P @ Rot.from_rotvec([0.3, -0.2, 0.1]).as_matrix().T
    P2, P2n = [], []
    for R, t, rng in _poses(30, 7):
        uv = _project(P, R, t)
        P2.append(uv)
        P2n.append(uv + rng.normal(0, 0.5, uv.shape))
    P2, P2n = np.array(P2), np.array(P2n)
    _check_batch(P[None], np.concatenate([P2, P2n]), 1e-9, shared=True)
    st = _check_batch(P[None, :4], P2[:, :4].copy(), 1e-9, shared=True)   # 4 coplanar points are enough there
    assert (st == 0).all()


def test_batch_mixed_conditioning_outliers_and_statuses_in_one_launch(cuda):
    """Noise-free, outlier-laden and near-planar problems and degenerate ones side by side in one launch: every problem
    is solved on its own, at its family's bar."""
    rng = np.random.default_rng(5)
    P = synth_kp3d(50)
    flat = P * np.array([1.0, 1.0, 0.06])
    P3, P2, fam = [], [], []
    for R, t, _ in _poses(20, 6):
        uv = _project(P, R, t) + rng.normal(0, 0.5, (50, 2))
        out = uv.copy()
        bad = rng.choice(50, 8, replace=False)
        out[bad] += rng.uniform(-80, 80, (8, 2))
        P3 += [P, P, flat]
        P2 += [_project(P, R, t), out, _project(flat, R, t) + rng.normal(0, 0.3, (50, 2))]
        fam += [1e-9, 1e-6, 2e-3]
    P3.append(np.zeros((50, 3)))                                    # all points at one place: degenerate (-2)
    P2.append(np.zeros((50, 2)))
    fam.append(0)
    P3, P2, fam = np.array(P3), np.array(P2), np.array(fam)
    R, t, st = (a.cpu().numpy() for a in solve_pnp_batch(P3, P2, CAM_K))
    assert st[-1] == -2 and np.isnan(R[-1]).all()
    hR, ht, hst = _host(P3[:-1], P2[:-1])
    assert (st[:-1] == 0).all() and (hst == 0).all()
    dR = np.abs(R[:-1] - hR).reshape(len(hR), -1).max(axis=1)
    dt = np.abs(t[:-1, :, 0] - ht).max(axis=1)
    assert (dR <= fam[:-1]).all() and (dt <= fam[:-1]).all(), (dR.max(), dt.max())


def test_batch_too_few_points_and_limits(cuda):
    P = synth_kp3d(50)
    uv = _project(P, np.eye(3), np.array([0, 0, 0.8]))
    _, _, st = solve_pnp_batch(P[:5], uv[None, :5], CAM_K)           # non-planar needs 6
    assert int(st[0]) == -1
    _, _, st = solve_pnp_batch(P[:3], uv[None, :3], CAM_K)
    assert int(st[0]) == -1
    big = np.concatenate([P, P[:15]])
    with pytest.raises(_lib.BetaposeHipError):
        solve_pnp_batch(big, _project(big, np.eye(3), np.array([0, 0, 0.8]))[None], CAM_K)


def test_batch_golden_frame_keypoints(cuda):
    """The reference's own post-NMS key points of the golden frames (random weights: no consistent projection), pruned
    to --left_keypoints 50 / 10 / 6."""
    from oracle import post_ref
    pipe = helpers.golden("pipeline.npz")
    for left in (50, 10, 6):
        P3, P2 = [], []
        for i in range(int(pipe["n_frames"])):
            kp, sc = pipe["f%d_nms_kp" % i], pipe["f%d_nms_score" % i][:, 0]
            k2, k3, _ = post_ref.prune_keypoints(kp, KP3D, sc, left)
            P3.append(k3); P2.append(k2)
        _check_batch(np.array(P3, np.float64), np.array(P2, np.float64), 1e-6)


# ---------------------------------------------------------------- the tail on records
def _record(rng, R, t, det=True):
    """A frame record whose 50 arg-max pixels come from projecting KP3D with (R, t) into a crop window (quantised to the
    heat-map grid, as a key-point net would emit them)."""
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
    hx = np.clip(np.round((uv[:, 0] - ul[0] + dx) * 80 / lenH - 0.2), 0, 63).astype(np.int32)
    hy = np.clip(np.round((uv[:, 1] - ul[1] + dy) * 80 / lenH - 0.2), 0, 79).astype(np.int32)
    kp = rec[16:].reshape(50, 6)
    kp[:, 0] = (hy * 64 + hx).astype(np.int32).view(np.float32)
    kp[:, 1] = rng.uniform(0.35, 0.95, 50).astype(np.float32)
    kp[:, 2:] = rng.uniform(0, 0.3, (50, 4)).astype(np.float32)
    return rec


def _records():
    """Hand-made records: every case the tail branches on."""
    recs = []
    for R, t, rng in _poses(6, 11):
        recs.append(_record(rng, R, t))
    rng = np.random.default_rng(3)
    R, t = np.eye(3), np.array([0.01, -0.02, 0.7])
    recs.append(_record(rng, R, t, det=False))                        # idx = -1: no detection
    r = _record(rng, R, t); r[16 + 1::6][:50] = 0.2; recs.append(r)    # every score below 0.3: dropped by pPose-NMS
    r = _record(rng, R, t); r[16 + 1::6][:50][[3, 9, 27]] = 0.0; recs.append(r)   # zero scores (1e-5, position gated)
    r = _record(rng, R, t); r[16 + 1::6][:50][10:30] = 0.5; recs.append(r)        # ties across the pruning cut
    r = _record(rng, R, t)                                             # maxima on the heat-map border
    kp = r[16:].reshape(50, 6)
    kp[:4, 0] = np.array([0, 63, 79 * 64, 79 * 64 + 63], np.int32).view(np.float32)
    kp[4:8, 0] = np.array([5 * 64, 5 * 64 + 63, 40, 79 * 64 + 20], np.int32).view(np.float32)
    recs.append(r)
    r = _record(rng, R, t); r[16 + 1::6][:50][[0, 1, 2]] = -0.4; recs.append(r)   # negative maxval
    r = _record(rng, R, t); r[16 + 2::6][:50] = r[16 + 3::6][:50]; recs.append(r)  # flat neighbours: sign 0
    return np.array(recs)


def _same_dict(a, b, tol, what=""):
    assert a.keys() == b.keys(), what
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
    assert a["cam_R"].shape == (3, 3) and a["cam_t"].shape == (3, 1)
    d = max(np.abs(a["cam_R"] - b["cam_R"]).max(), np.abs(a["cam_t"] - b["cam_t"]).max())
    assert d <= tol, (what, d)


def _compare_rows(recs, rows, kp3d, left, tol, names=None):
    from betapose_amd.pipeline import finish_pose_record, finish_record
    n_pose = 0
    for i, (rec, row) in enumerate(zip(recs, rows)):
        name = names[i] if names else "%04d.png" % i
        try:
            want = finish_record(rec, name, kp3d, CAM_K, left)
        except _lib.BetaposeHipError:
            with pytest.raises(_lib.BetaposeHipError):
                finish_pose_record(rec, row, name)
            assert row[0] < 0
            continue
        got = finish_pose_record(rec, row, name)
        _same_dict(got, want, tol, "frame %d left %d" % (i, left))
        if want["result"]:
            assert int(row[1]) == min(50, left)
            n_pose += 1
    return n_pose


@pytest.mark.parametrize("left", [50, 10, 6, 4, 0])
def test_pose_from_records_matches_finish_record(cuda, left):
    recs = _records()
    rows = ops.pose_from_records(torch.from_numpy(recs).cuda(), KP3D, CAM_K, left).cpu().numpy()
    st = rows[:, 0]
    assert st[6] == 1 and st[7] == 2
    if left >= 6:
        assert (st[:6] == 0).all()
    else:
        assert (st[:6] == -1).all()                                   # n < 6 non-planar: the host raises too
    _compare_rows(recs, rows, KP3D, left, 1e-6)


def test_pose_from_records_rejects_bad_arguments(cuda):
    recs = torch.from_numpy(_records()).cuda()
    with pytest.raises(_lib.BetaposeHipError):
        ops.pose_from_records(recs, KP3D[:40], CAM_K)
    with pytest.raises(_lib.BetaposeHipError):
        ops.pose_from_records(recs, KP3D, CAM_K, -1)


# ---------------------------------------------------------------- in the frame pipeline
def _engines(max_batch, mode):
    from betapose_amd.darknet import Darknet
    from betapose_amd.kpd import FastPoseHIP
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416, max_batch=max_batch).load_stream(helpers.yolo_stream()).cuda()
    pose = FastPoseHIP(helpers.kpd_state_dict(), n_classes=50, max_batch=max_batch).cuda()
    det.set_precision(mode)
    pose.set_precision(mode)
    return det, pose


@pytest.fixture(scope="module")
def frames64():
    return synth.synth_frames(64, helpers.FRAME_SEED)


@pytest.mark.parametrize("mode,batch", [("bf16x3", 1), ("bf16x3", 28), ("f16", 1), ("f16", 28)])
def test_pipeline_with_pose_solver(cuda, frames64, mode, batch):
    """sweep64's 64 frames through the pipeline with and without the tail: records bit-identical, one more launch
    while the solver is on, the pose rows equal to the host tail at the bars."""
    from betapose_amd.pipeline import FramePipeline
    det, pose = _engines(batch, mode)
    pipe = FramePipeline(det, pose, 480, 640, batch=batch)
    launches = [np.stack(frames64[i:i + batch]) for i in range(0, 64 - batch + 1, batch)]
    plain = [pipe.run(f) for f in launches]
    n0 = pipe.kernel_count()
    pipe.set_pose_solver(KP3D, CAM_K, 10)
    recs, rows = [], []
    for f in launches:
        recs.append(pipe.run(f))
        rows.append(pipe.poses.cpu().numpy())
    assert pipe.kernel_count() == n0 + 1
    for a, b in zip(plain, recs):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    n_pose = _compare_rows(np.concatenate(recs), np.concatenate(rows), KP3D, 10, 1e-6)
    assert n_pose > 0
    pipe.set_pose_solver(None)
    again = pipe.run(launches[0])
    assert pipe.kernel_count() == n0
    np.testing.assert_array_equal(again.view(np.int32), plain[0].view(np.int32))


def test_pose_rows_deterministic_across_replays_and_streams(cuda):
    from betapose_amd.pipeline import FramePipeline
    det, pose = _engines(1, "bf16x3")
    pipe = FramePipeline(det, pose, 480, 640, batch=1).set_pose_solver(KP3D, CAM_K, 50)
    frame = synth.synth_frames(1, 99)[0]
    pipe.run(frame)
    a = pipe.poses.cpu().numpy().copy()
    pipe.run(frame)
    b = pipe.poses.cpu().numpy().copy()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        pipe.enqueue(s.cuda_stream)
    s.synchronize()
    c = pipe.poses.cpu().numpy().copy()
    assert a[0, 0] == 0
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))
    np.testing.assert_array_equal(a.view(np.int64), c.view(np.int64))
    recs = torch.from_numpy(np.repeat(pipe.results.cpu().numpy(), 5, axis=0)).cuda()
    rows = ops.pose_from_records(recs, KP3D, CAM_K, 50).cpu().numpy()   # the tail alone, five copies in one launch
    for r in rows:
        np.testing.assert_array_equal(r.view(np.int64), a[0].view(np.int64))


def _write_pngs(tmp_path, frames):
    from PIL import Image
    paths = []
    for i, fr in enumerate(frames):
        p = tmp_path / ("%04d.png" % i)
        Image.fromarray(fr[:, :, ::-1].copy()).save(p, compress_level=1)
        paths.append(str(p))
    return paths


def test_streamed_runner_with_pose_solver(tmp_path, cuda):
    from betapose_amd.frame_loader import FrameLoader
    from betapose_amd.pipeline import StreamedRunner
    frames = synth.synth_frames(7, 321)
    paths = _write_pngs(tmp_path, frames)
    det, pose = _engines(2, "bf16x3")
    runner = StreamedRunner(det, pose, 480, 640, streams=3, batch=2, pose_solver=(KP3D, CAM_K, 10))
    got = {}
    ld = FrameLoader(paths, threads=2, depth=8)
    assert runner.run(ld, lambda i, rec, row: got.__setitem__(i, (rec, row))) == 7
    ld.close()
    assert list(got) == list(range(7))
    recs = np.array([got[i][0] for i in range(7)])
    rows = np.array([got[i][1] for i in range(7)])
    assert _compare_rows(recs, rows, KP3D, 10, 1e-6) > 0


def test_multi_object_runner_with_pose_solvers(tmp_path, cuda):
    from betapose_amd.darknet import Darknet
    from betapose_amd.frame_loader import FrameLoader
    from betapose_amd.kpd import FastPoseHIP
    from betapose_amd.pipeline import MultiObjectRunner
    from betapose_amd.weights import fastpose_stream_from_state_dict
    frames = synth.synth_frames(3, 77)
    paths = _write_pngs(tmp_path, frames)
    engines, kp = {}, {1: KP3D, 5: synth_kp3d(50, seed=11)}
    for o in (1, 5):
        sy, sk = synth.object_seeds(o)
        det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416).load_stream(synth.synth_yolo_stream(sy)).cuda()
        pose = FastPoseHIP.from_stream(fastpose_stream_from_state_dict(synth.synth_fastpose_state_dict(sk, 50), 50),
                                       n_classes=50).cuda()
        engines[o] = (det, pose)
    runner = MultiObjectRunner(engines, [1, 5], 480, 640, streams=2,
                               pose_solvers={o: (kp[o], CAM_K, 50) for o in (1, 5)})
    got = {}
    ld = FrameLoader(paths, threads=2, depth=8)
    assert runner.run(ld, [0, 1, 2], lambda u: True, lambda u, rec, row: got.__setitem__(u, (rec, row))) == 6
    ld.close()
    for u, (rec, row) in got.items():
        _compare_rows(rec[None], row[None], kp[(1, 5)[u % 2]], 50, 1e-6)


# ---------------------------------------------------------------- harnesses
def _run(args):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _json_pair(a, b, tol):
    ja, jb = json.load(open(a)), json.load(open(b))
    assert len(ja) == len(jb)
    for x, y in zip(ja, jb):
        assert x["image_id"] == y["image_id"] and x["keypoints"] == y["keypoints"] and x["score"] == y["score"]
        assert np.abs(np.subtract(x["cam_R"], y["cam_R"])).max() <= tol
        assert np.abs(np.subtract(x["cam_t"], y["cam_t"])).max() <= tol


def test_evaluate_synthetic_device_pnp(tmp_path):
    outs = {}
    for flag in ([], ["--device_pnp"]):
        od = tmp_path / ("dev" if flag else "host")
        outs[bool(flag)] = _run([os.path.join(ROOT, "evaluate.py"), "--synthetic", "16", "--outdir", str(od), "--fused",
                                 "--left_keypoints", "10"] + flag)
    poses = [re.search(r"(\d+) with a pose", outs[k]).group(1) for k in (False, True)]
    assert poses[0] == poses[1] and int(poses[0]) > 0
    _json_pair(tmp_path / "host" / "Betapose-results.json", tmp_path / "dev" / "Betapose-results.json", 1e-6)


@pytest.mark.parametrize("occlusion", [False, True])
def test_sixd_harness_device_pnp_accuracy_lines(tmp_path, cuda, occlusion):
    """A small synthetic SIXD tree (test_gpu_harness.py's closed loop): the ADD / 2-D / IoU lines are the same with and
    without --device_pnp."""
    from betapose_amd.pipeline import FramePipeline, finish_record
    obj_id = 1
    frames = helpers.frames(3)
    indir = tmp_path / "rgb"
    indir.mkdir()
    _write_pngs(indir, frames)
    kp_mm = np.round(synth_kp3d(50) * 1000.0, 6)
    det, pose = _engines(1, "bf16x3")
    pipe = FramePipeline(det, pose, 480, 640, batch=1, confidence=0.01)
    gt, rng = {}, np.random.default_rng(4)
    for i, fr in enumerate(frames):
        out = finish_record(pipe.run(fr)[0], "%04d.png" % i, kp_mm / 1000.0, CAM_K, 10)
        x1, y1, x2, y2 = [float(v) for v in out["result"][0]["bbox"]]
        t = np.asarray(out["cam_t"]).reshape(3) * 1000.0 + rng.normal(0, 3.0, 3)     # some poses miss the ADD bar
        mine = (obj_id, out["cam_R"], t, [x1, y1, x2 - x1, y2 - y1])
        gt[i] = [(7, np.eye(3), np.array([0.0, 0.0, 800.0]), [5, 5, 20, 20]), mine] if occlusion else [mine]
    del pipe, det, pose
    synth.write_sixd_tree(str(tmp_path / "sixd"), 2 if occlusion else obj_id, gt,
                          {obj_id: np.random.default_rng(0).normal(size=(300, 3)) * 30.0}, {obj_id: kp_mm}, {obj_id: 100.0})
    script = "occlusion_evaluate.py" if occlusion else "evaluate.py"
    lines = {}
    for flag in ([], ["--device_pnp"]):
        od = tmp_path / ("dev" if flag else "host")
        out = _run([os.path.join(ROOT, script), "--indir", str(indir), "--outdir", str(od), "--sixd_base",
                    str(tmp_path / "sixd"), "--synth_weights", "--left_keypoints", "10"] +
                   (["--obj_ids", str(obj_id)] if occlusion else ["--obj_id", str(obj_id), "--fused"]) + flag)
        lines[bool(flag)] = re.findall(r"(?:Mean add accuracy|2d reprojection accuracy|Mean IoU).* for seq \d+ is: \S+", out)
    assert len(lines[False]) == 3 and lines[False] == lines[True], lines
