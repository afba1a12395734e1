"""bp_pose_errors (csrc/pose_metrics.hip): ADD, ADD-S and the 2-D projection error of many pose pairs in one launch,
f64, against the host numpy definitions (metrics.add_err / add_s_err / projection_error_2d), analytic cases on a large
lattice, run-to-run determinism, argument checks, evaluate_results on the device and the harness's --symmetric_ids."""
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


def device_errors(model, gt, est, cam=CAM, want=7, stream=None):
    import torch
    from betapose_amd import _lib
    d_model = torch.from_numpy(np.ascontiguousarray(model, np.float64)).cuda()
    d_gt = torch.from_numpy(np.ascontiguousarray(gt[:, :3, :4].reshape(-1, 12))).cuda()
    d_est = torch.from_numpy(np.ascontiguousarray(est[:, :3, :4].reshape(-1, 12))).cuda()
    d_out = torch.full((len(gt), 3), -1.0, dtype=torch.float64, device="cuda")
    K = np.ascontiguousarray(cam, np.float64).reshape(9)
    s = stream if stream is not None else torch.cuda.current_stream()
    _lib.check(_lib.lib().bp_pose_errors(_lib.ptr(d_model), len(model), _lib.ptr(d_gt), _lib.ptr(d_est), len(gt),
                                         _lib.ptr(K), want, _lib.ptr(d_out), s.cuda_stream))
    return d_out.cpu().numpy()


def host_errors(model, gt, est, cam=CAM):
    from betapose_amd import metrics
    return np.stack(metrics.pose_errors(gt, est, model, cam), axis=1)


@pytest.mark.parametrize("P", [1, 3, 37])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_pose_errors_match_numpy(cuda, n, P):
    rng = np.random.default_rng(1000 * n + P)
    model = rng.normal(size=(n, 3)) * [0.05, 0.04, 0.03]
    gt, est = linemod_poses(rng, P)
    dev = device_errors(model, gt, est)
    ref = host_errors(model, gt, est)
    assert np.abs(dev[:, :2] - ref[:, :2]).max() < 1e-12, np.abs(dev[:, :2] - ref[:, :2]).max()
    assert np.abs(dev[:, 2] - ref[:, 2]).max() < 1e-9
    assert (dev[:, 1] <= dev[:, 0] + 1e-15).all()


def lattice(h=1e-3, m=147):
    """m x m square lattice of spacing h in the z = 0 plane, centred on the z axis (21 609 points)."""
    c = (np.arange(m) - (m - 1) / 2) * h
    x, y = np.meshgrid(c, c, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(m * m)], axis=1)


def test_lattice_shift_and_quarter_turn(cuda):
    rng = np.random.default_rng(7)
    model = lattice()
    P = 4
    gt, _ = linemod_poses(rng, P)
    # shift along the model's x axis by delta < h / 2: every vertex's closest estimated vertex is its own
    delta = 3.1e-4
    shift = np.eye(4)
    shift[0, 3] = delta
    dev = device_errors(model, gt, gt @ shift, want=3)
    assert np.abs(dev[:, 0] - delta).max() < 1e-12 and np.abs(dev[:, 1] - delta).max() < 1e-12
    assert (dev[:, 2] == -1.0).all()          # unrequested column untouched
    # a quarter turn about z maps the lattice onto itself
    rz = np.eye(4)
    rz[:2, :2] = [[np.cos(np.pi / 2), -np.sin(np.pi / 2)], [np.sin(np.pi / 2), np.cos(np.pi / 2)]]
    dev = device_errors(model, gt, gt @ rz)
    assert dev[:, 1].max() <= 1e-12
    want_add = float(np.mean(np.sqrt(2.0) * np.linalg.norm(model[:, :2], axis=1)))
    assert np.abs(dev[:, 0] - want_add).max() < 1e-12


def test_bit_identical_across_calls_and_streams(cuda):
    import torch
    rng = np.random.default_rng(11)
    model = rng.normal(size=(4099, 3)) * 0.05
    gt, est = linemod_poses(rng, 1500)
    a = device_errors(model, gt, est)
    b = device_errors(model, gt, est)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c = device_errors(model, gt, est, stream=s1)
    d = device_errors(model, gt, est, stream=s2)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert np.array_equal(a.view(np.int64), c.view(np.int64))
    assert np.array_equal(a.view(np.int64), d.view(np.int64))


def test_bad_arguments(cuda):
    import torch
    from betapose_amd import _lib
    L = _lib.lib()
    m = torch.zeros(10, 3, dtype=torch.float64, device="cuda")
    g = torch.zeros(2, 12, dtype=torch.float64, device="cuda")
    out = torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    K = np.ascontiguousarray(CAM).reshape(9)
    mp, gp, op, kp = m.data_ptr(), g.data_ptr(), out.data_ptr(), K.ctypes.data
    cases = [((mp, 0, gp, gp, 2, kp, 7, op), "positive"), ((mp, -3, gp, gp, 2, kp, 7, op), "positive"),
             ((mp, 10, gp, gp, 0, kp, 7, op), "positive"), ((None, 10, gp, gp, 2, kp, 7, op), "null"),
             ((mp, 10, None, gp, 2, kp, 7, op), "null"), ((mp, 10, gp, None, 2, kp, 7, op), "null"),
             ((mp, 10, gp, gp, 2, kp, 7, None), "null"), ((mp, 10, gp, gp, 2, None, 4, op), "K is required"),
             ((mp, 10, gp, gp, 2, kp, 0, op), "want")]
    for args, text in cases:
        assert L.bp_pose_errors(*args, None) < 0, args
        assert text in L.bp_last_error().decode(), (args, L.bp_last_error())
    assert L.bp_pose_errors(mp, 10, gp, gp, 2, None, 3, op, None) == 0     # K may be NULL without the 2-D column


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
    synth.write_sixd_tree(str(tmp_path), 1, gt_by, {1: model_mm}, {1: half[:50]}, {1: 100.0})
    frames, model, _, diameter, cam = evaluate.load_sixd_gt(str(tmp_path), 1)
    # no error within 1e-9 of a threshold
    gts = np.stack([frames[nr][0]["pose"] for nr in range(40)])
    ests = np.stack([np.vstack((np.hstack((f["cam_R"], f["cam_t"])), [0, 0, 0, 1])) for f in final_result])
    add, adds, proj = metrics.pose_errors(gts, ests, model, cam)
    assert np.abs(add * 1000 - diameter / 10).min() > 1e-9 and np.abs(adds * 1000 - diameter / 10).min() > 1e-9
    assert np.abs(proj - 5.0).min() > 1e-9
    host = metrics.evaluate_results(final_result, frames, model, cam, diameter, symmetric=True)
    dev = metrics.evaluate_results(final_result, frames, model, cam, diameter, symmetric=True, device=cuda)
    assert set(host) == set(dev)
    for k in ("mean_add", "mean_2d_acc", "mean_iou", "mean_adds", "n"):
        assert host[k] == dev[k], k
    for k in ("mean_add_err_mm", "mean_adds_err_mm"):
        assert abs(host[k] - dev[k]) < 1e-9, k
    assert 0 < host["mean_add"] < host["mean_adds"]


METRIC_LINE = re.compile(r"^(Mean add accuracy|Mean add-s accuracy|2d reprojection accuracy|Mean IoU) for seq (\d+) is: (\S+)$",
                         re.M)


def test_harness_symmetric_ids(tmp_path, cuda):
    """evaluate.py on frame files + a SIXD tree whose ground truth is the pipeline's own poses: frame 0 as estimated,
    frame 1 turned half-way about the (half-turn symmetric) model's z axis, frame 2 moved 30 cm.  --symmetric_ids 1 adds
    the ADD-S line with the host metric's value; without the flag the metric lines are the three of before."""
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
                          {obj_id: kp_mm}, {obj_id: 100.0})

    def run(extra, name):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--indir", str(indir), "--outdir", str(out),
                            "--sixd_base", str(tmp_path / "sixd"), "--synth_weights", "--fused", "--obj_id", str(obj_id)]
                           + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout, json.loads(open(out / "Betapose-results.json").read())

    plain, _ = run([], "plain")
    assert [m[0] for m in METRIC_LINE.findall(plain)] == ["Mean add accuracy", "2d reprojection accuracy", "Mean IoU"]
    assert "add-s" not in plain
    sym, res = run(["--symmetric_ids", "1"], "sym")
    lines = METRIC_LINE.findall(sym)
    assert [m[0] for m in lines] == ["Mean add accuracy", "Mean add-s accuracy", "2d reprojection accuracy", "Mean IoU"]
    assert [m for m in lines if m[0] != "Mean add-s accuracy"] == METRIC_LINE.findall(plain)

    import evaluate
    frames_gt, model, _, diameter, cam = evaluate.load_sixd_gt(str(tmp_path / "sixd"), obj_id)
    final_result = [{"imgname": r_["image_id"], "cam_R": np.array(r_["cam_R"]).reshape(3, 3),
                     "cam_t": np.array(r_["cam_t"]).reshape(3, 1), "result": [{"bbox": boxes[r_["image_id"]]}]}
                    for r_ in res]
    host = metrics.evaluate_results(final_result, frames_gt, model, cam, diameter, symmetric=True)
    assert dict((m[0], m[2]) for m in lines)["Mean add-s accuracy"] == "%.3f" % host["mean_adds"]
    assert "%.3f" % host["mean_adds"] == "0.667" and "%.3f" % host["mean_add"] == "0.333"
