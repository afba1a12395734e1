"""Candidate boxes per frame on the GPU: select with box NMS (csrc/yolo_tail.hip) against tests/nms_ref.py, the
candidate crop, ``CandidatePipeline`` against the stand-alone stages and against ``FramePipeline`` at one candidate, and
the candidate pose tail (csrc/pose_tail_cands.hip) against ``pipeline.finish_candidate_records``.

Bars: everything but R, t is bit-identical.  R, t of the candidate tail: 1e-9, the bar tests/test_gpu_pose_tail.py holds
the iterative tail to on noise-free problems."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers  # noqa: E402
import nms_ref  # noqa: E402
from betapose_amd import _lib, ops, synth  # noqa: E402
from betapose_amd.darknet import Darknet  # noqa: E402
from betapose_amd.eval import decode_keypoints  # noqa: E402
from betapose_amd.kpd import FastPoseHIP  # noqa: E402
from betapose_amd.pipeline import (CandidatePipeline, FramePipeline, finish_candidate_pose_record,  # noqa: E402
                                   finish_candidate_records)
from betapose_amd.synth import CAM_K, synth_kp3d  # noqa: E402

KP3D = synth_kp3d(50)
F32 = np.float32
NMS_CONF = 0.45
RT_TOL = 1e-9


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ------------------------------------------------------------------ select, tensor form
def _other_row(rows):
    return 3 if rows <= 2000 else 2049


def _planted(rows, rng):
    """[2][rows][7] (two classes): image 1 has no live row (every objectness below conf = 0.5); image 0 carries, with
    pairwise distinct objectness in planting order (highest first):
      A  40 x 40 at x = 100, in the LAST row (the highest stride of its thread)
      B  the same box at x = 112: IoU with A above the threshold -> removed by A
      C  the same box at x = 124: IoU with B above, with A below the threshold -> kept (the chain keeps A and C)
      nine 30 x 30 boxes far apart, in rows of different threads' strides and different waves -> all kept
      one row of class 1 with the highest objectness of all -> never a candidate of class 0."""
    pred = np.zeros((2, rows, 7), F32)
    pred[:, :, :4] = rng.uniform(5, 400, (2, rows, 4))
    pred[:, :, 4] = rng.uniform(0.0, 0.4, (2, rows))
    pred[:, :, 5], pred[:, :, 6] = 0.9, 0.5
    obj = iter(np.linspace(0.99, 0.6, 40).astype(F32))

    def put(r, cx, cy, w, h):
        pred[0, r, :5] = [cx, cy, w, h, next(obj)]
    put(rows - 1, 100, 100, 40, 40)
    put(1, 112, 100, 40, 40)
    put(rows // 2, 124, 100, 40, 40)
    spots = [(300, 60), (300, 200), (300, 340), (60, 300), (200, 300), (380, 380), (30, 30), (200, 30), (30, 200)]
    for i, (cx, cy) in enumerate(spots):
        put((37 + i * 1031) % rows if rows > 2000 else (7 + i * 11) % (rows - 2) + 2, cx, cy, 30, 30)
    pred[0, _other_row(rows)] = [250, 250, 30, 30, 0.995, 0.1, 0.8]
    return pred


@pytest.mark.parametrize("rows", [96, 1024, 2500, 10647])
def test_select_nms_tensor_form_matches_restatement(cuda, rows):
    pred = _planted(rows, np.random.default_rng(rows))
    other = _other_row(rows)
    live = pred[0, :, 4] > 0.5
    assert len(np.unique(pred[0, live, 4])) == int(live.sum())       # precondition: objectness pairwise distinct
    single = np.zeros((2, rows, 7), F32)
    single[:] = pred
    single[0, :, 4] = np.where(np.arange(rows) == rows - 1, pred[0, :, 4], 0.0)   # one live row
    for name, t in (("planted", pred), ("one live row", single)):
        for Cn in (1, 3, 8):
            ious = []
            want, wcnt = nms_ref.select_nms(t, 0.5, 80, NMS_CONF, Cn, ious_out=ious)
            for v in ious:                                           # precondition: no executed IoU near the threshold
                assert np.all(np.abs(v - F32(NMS_CONF)) > 1e-6)
            sel, cnt = ops.select_nms(torch.from_numpy(t).to(cuda), Cn, NMS_CONF, confidence=0.5)
            np.testing.assert_array_equal(cnt.cpu().numpy(), wcnt, err_msg="%s C=%d" % (name, Cn))
            np.testing.assert_array_equal(_bits(sel.cpu().numpy()), _bits(want), err_msg="%s C=%d" % (name, Cn))
            if name == "planted":
                assert wcnt[0] == min(Cn, 11) and wcnt[1] == 0        # A, C and the nine spots survive; B and the other class do not
                idx = want[0, :wcnt[0], 0].view(np.int32)
                assert idx[0] == rows - 1 and other not in idx and 1 not in idx
                if Cn >= 2:
                    assert idx[1] == rows // 2                        # the chain keeps A and C
                one = ops.select_nms(torch.from_numpy(t).to(cuda), 1, NMS_CONF, confidence=0.5)[0][:, 0]
                plain = torch.empty((2, 8), device=cuda)
                _lib.check(_lib.lib().bp_yolo_select(torch.from_numpy(t).to(cuda).data_ptr(), 2, rows, 7, 0.5, 80, plain.data_ptr(),
                                                     _lib.current_stream()))
                np.testing.assert_array_equal(_bits(one.cpu().numpy()), _bits(plain.cpu().numpy()))
            else:
                assert wcnt[0] == 1
    # the other class as the one asked for
    want, wcnt = nms_ref.select_nms(pred, 0.5, 80, NMS_CONF, 3, class_id=1)
    sel, cnt = ops.select_nms(torch.from_numpy(pred).to(cuda), 3, NMS_CONF, class_id=1, confidence=0.5)
    assert wcnt[0] == 1 and int(want[0, 0, :1].view(np.int32)[0]) == other
    np.testing.assert_array_equal(_bits(sel.cpu().numpy()), _bits(want))
    np.testing.assert_array_equal(cnt.cpu().numpy(), wcnt)


# ------------------------------------------------------------------ engines
@pytest.fixture(scope="module")
def nets(cuda):
    from betapose_amd import cfg as Cf
    blocks = Cf.parse_cfg_text(Cf.yolov3_single_cfg_text())
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416, max_batch=2).load_stream(synth.synth_yolo_stream(1, blocks)).cuda()
    pose = FastPoseHIP(synth.synth_fastpose_state_dict(2), max_batch=4).cuda()
    return det, pose


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
def test_select_nms_head_form_matches_restatement(nets, cuda, prec):
    det, _ = nets
    det.set_precision(prec)
    try:
        x = torch.cat([helpers.yolo_input_from_frame(f) for f in helpers.frames(2)]).to(cuda)
        pred = det.forward(x)
        conf = float(torch.quantile(pred[0, :, 4], 0.6))             # thousands of live rows
        assert int((pred[:, :, 4] > conf).sum()) > 2000
        p = pred.cpu().numpy()
        for Cn in (1, 8):
            want, wcnt = nms_ref.select_nms(p, conf, 80, NMS_CONF, Cn)
            sel, cnt = det.forward_select_nms(x, Cn, NMS_CONF, confidence=conf)
            np.testing.assert_array_equal(cnt.cpu().numpy(), wcnt)
            np.testing.assert_array_equal(_bits(sel.cpu().numpy()), _bits(want))
            sel2, cnt2, pred2 = det.forward_select_nms(x, Cn, NMS_CONF, confidence=conf, want_pred=True)
            assert torch.equal(sel2.view(torch.int32), sel.view(torch.int32)) and torch.equal(cnt2, cnt) and torch.equal(pred2, pred)
            plain = det.forward_select(x, confidence=conf)
            assert torch.equal(sel[:, 0].contiguous().view(torch.int32), plain.view(torch.int32))
    finally:
        det.set_precision("bf16x3")


def test_crop_candidates_matches_crop(cuda):
    rng = np.random.default_rng(5)
    frames = torch.from_numpy(np.stack([synth.synth_frame(40 + i) for i in range(2)])).to(cuda)
    Cn = 3
    sel = np.zeros((2 * Cn, 8), F32)
    for n in range(2 * Cn):
        x1, y1 = rng.uniform(0, 250, 2)
        sel[n, 1:5] = [x1, y1, x1 + rng.uniform(20, 150), y1 + rng.uniform(20, 150)]
    sel[4] = 0
    sel[4, 0] = np.array([-1], np.int32).view(F32)[0]                # a slot without a box
    sel_t = torch.from_numpy(sel).to(cuda)
    got, pts = ops.crop_candidates(frames, Cn, sel=sel_t)
    for n in range(2 * Cn):
        want, wpts = ops.crop(frames[n // Cn:n // Cn + 1], sel=sel_t[n:n + 1])
        assert torch.equal(got[n:n + 1], want) and torch.equal(pts[n:n + 1], wpts), n
    nodet, npts = ops.crop(frames[1:2], sel=torch.from_numpy(sel[4:5]).to(cuda))
    assert torch.equal(got[4:5], nodet)


def test_candidate_pipeline_consistency(nets, cuda):
    det, pose = nets
    frame = helpers.frames(1)[0]
    conf = 0.01
    cp = CandidatePipeline(det, pose, 480, 640, candidates=4, nms_conf=NMS_CONF, confidence=conf, use_graph=False)
    eager, n_eager = cp.run(frame)
    assert 1 <= n_eager <= 4
    # every row = the stand-alone stages at batch 4 on the selected boxes
    fr = torch.from_numpy(frame[None]).to(cuda)
    inps, pts = ops.crop_candidates(fr, 4, sel=torch.from_numpy(eager[:, :8].copy()).to(cuda))
    kp = torch.empty((4, 50, 6), device=cuda)
    _lib.check(_lib.lib().bp_kpd_forward_argmax(pose.handle, inps.data_ptr(), 4, None, kp.data_ptr(), _lib.current_stream()))
    np.testing.assert_array_equal(_bits(eager[:, 8:16]), _bits(pts.cpu().numpy()))
    np.testing.assert_array_equal(_bits(eager[:, 16:]), _bits(kp.cpu().numpy().reshape(4, 300)))
    cg = CandidatePipeline(det, pose, 480, 640, candidates=4, nms_conf=NMS_CONF, confidence=conf, use_graph=True).prepare()
    for _ in range(2):
        replay, n_replay = cg.run(frame)
        assert n_replay == n_eager
        np.testing.assert_array_equal(_bits(replay), _bits(eager))
    fp = FramePipeline(det, pose, 480, 640, batch=1, confidence=conf).prepare()
    # candidate 0 is FramePipeline's box: select record and crop window bit for bit.  Its key-point slots are NOT compared
    # here: the key-point net's launch plan depends on the batch (split-K, fusion), so a batch-4 pass sums in another order
    # than the batch-1 pass; they are held to bp_kpd_forward_argmax at batch 4 above, and to FramePipeline at C = 1 below
    np.testing.assert_array_equal(_bits(fp.run(frame)[0, :16]), _bits(eager[0, :16]))
    c1 = CandidatePipeline(det, pose, 480, 640, candidates=1, nms_conf=NMS_CONF, confidence=conf).prepare()
    # launches: 2 resize + the detector's with its select + 1 crop + the key-point net's with its arg-max at
    # batch C, i.e. FramePipeline's count at batch 1 with the key-point net's launches taken at batch C instead of 1
    L = _lib.lib()
    k1, k4 = L.bp_kpd_launch_count(pose.handle, 1), L.bp_kpd_launch_count(pose.handle, 4)
    assert k1 > 100 and k4 > 100
    assert c1.kernel_count() == fp.kernel_count() > k1
    n4 = cg.kernel_count()
    assert n4 == fp.kernel_count() - k1 + k4
    cg.set_pose_solver(KP3D, CAM_K, 50).prepare()
    assert cg.kernel_count() == n4 + 1                                # the pose tail is one more node


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
def test_one_candidate_is_frame_pipeline(nets, cuda, prec):
    det, pose = nets
    det.set_precision(prec)
    pose.set_precision(prec)
    try:
        for i, frame in enumerate(helpers.frames(2)):
            fp = FramePipeline(det, pose, 480, 640, batch=1).set_pose_solver(KP3D, CAM_K, 10)
            want = fp.run(frame)[0]
            wpose = fp.poses.cpu().numpy()[0]
            cp = CandidatePipeline(det, pose, 480, 640, candidates=1, nms_conf=NMS_CONF).set_pose_solver(KP3D, CAM_K, 10)
            got, n = cp.run(frame)
            assert n == 1
            np.testing.assert_array_equal(_bits(got[0]), _bits(want))
            np.testing.assert_array_equal(cp.poses.cpu().numpy()[0].view(np.int64), wpose.view(np.int64))
    finally:
        det.set_precision("bf16x3")
        pose.set_precision("bf16x3")


# ------------------------------------------------------------------ candidate pose tail against the host
def _base_record(rng, scores=(0.35, 0.95), box=None):
    """A record whose 50 arg-max pixels project KP3D with a fixed pose into a 200 x 250 crop window (lenH = 250)."""
    from scipy.spatial.transform import Rotation as Rot
    R = Rot.from_rotvec([0.3, -0.5, 0.2]).as_matrix()
    t = np.array([0.02, -0.03, 0.8])
    Y = KP3D @ R.T + t
    uv = (Y @ CAM_K.T)
    uv = uv[:, :2] / uv[:, 2:]
    rec = np.zeros(316, F32)
    rec[0] = np.array([5], np.int32).view(F32)[0]
    c = uv.mean(axis=0)
    ul = np.round(c - np.array([110.0, 130.0])).astype(F32)
    br = ul + np.array([200.0, 250.0], F32)
    rec[1:5] = [10, 20, 30, 40]
    rec[5] = 0.875
    rec[8:10], rec[10:12] = ul, br
    rec[12:16] = [ul[0] + 5, ul[1] + 7, br[0] - 4, br[1] - 6] if box is None else box
    hx = np.clip(np.round((uv[:, 0] - ul[0]) * 80 / 250 - 0.2), 1, 62).astype(np.int32)
    hy = np.clip(np.round((uv[:, 1] - ul[1]) * 80 / 250 - 0.2), 1, 78).astype(np.int32)
    kp = rec[16:].reshape(50, 6)
    kp[:, 0] = (hy * 64 + hx).astype(np.int32).view(F32)
    kp[:, 1] = rng.uniform(scores[0], scores[1], 50).astype(F32)
    kp[:, 2:] = rng.uniform(0, 0.3, (50, 4)).astype(F32)
    return rec


def _shifted(base, rng, dx, dy, stretch, scores):
    """``base`` seen through a crop window moved by (dx, dy) px and stretched by ``stretch``: every key point moves by
    (dx, dy) plus a per-point offset that grows with its heat-map position (at most 250 * stretch px)."""
    r = base.copy()
    r[8] += F32(dx); r[9] += F32(dy)
    r[10] = r[8] + F32(200.0 * (1 + stretch)); r[11] = r[9] + F32(250.0 * (1 + stretch))
    r[16 + 1::6][:50] = rng.uniform(scores[0], scores[1], 50).astype(F32)
    return r


SMALL_BOX = [300.0, 200.0, 330.0, 222.0]      # longer side 30 px: ref_dist = 3


def _case(kind, n, seed):
    rng = np.random.default_rng(seed)
    small = kind in ("simi", "below")
    base = _base_record(rng, scores=(0.8, 0.95), box=SMALL_BOX if small else None)   # candidate 0 has the highest mean score
    recs = [base]
    for c in range(1, n):
        lo = (0.35, 0.7)
        if kind == "coincident":
            a = 2 * np.pi * c / n
            recs.append(_shifted(base, rng, 0.2 * np.cos(a), 0.2 * np.sin(a), 2e-5 * c, lo))
        elif kind == "far":
            recs.append(_shifted(base, rng, 120.0 * c, 0.0, 2e-5 * c, lo))
        elif kind == "simi":
            a = 2 * np.pi * c / n
            recs.append(_shifted(base, rng, 3.2 * np.cos(a), 3.2 * np.sin(a), 2e-5 * c, lo))
        elif kind == "below":
            recs.append(_shifted(base, rng, 4.0 * c, 0.0, 2e-5 * c, lo))
    return np.array(recs)


def _cases():
    out = []
    for kind in ("coincident", "far", "simi", "below"):
        for n in (2, 3, 8):
            out.append(("%s n=%d" % (kind, n), _case(kind, n, 100 + n)))
    rng = np.random.default_rng(9)
    base = _base_record(rng, scores=(0.8, 0.95))
    mixed = [base, _shifted(base, rng, 0.15, 0.1, 2e-5, (0.35, 0.7)), _shifted(base, rng, -0.1, 0.2, 4e-5, (0.35, 0.7)),
             _shifted(base, rng, 150.0, 0.0, 0.0, (0.5, 0.75)), _shifted(base, rng, 150.2, 0.1, 2e-5, (0.35, 0.6))]
    out.append(("two clusters", np.array(mixed)))
    weak = _base_record(rng, scores=(0.29, 0.29))                    # the highest mean, no score reaches 0.3: filtered
    other = _shifted(base, rng, 150.0, 0.0, 0.0, (0.1, 0.1))
    other[16 + 1::6][:50][:6] = 0.9                                  # mean 0.196, maximum 0.9: kept
    out.append(("first pick filtered", np.array([weak, other])))
    return out


def _host_nms(recs):
    """bp_pose_nms on the decoded candidates + an f32 restatement of the greedy loop for the margins and the cluster of
    result[0]: -> (m, pick, pose, score, prop, mask of merged pose j, min margins)."""
    n = len(recs)
    kp = recs[:, 16:].reshape(n, 50, 6)
    _, preds, sc = decode_keypoints(kp, recs[:, 8:10], recs[:, 10:12])
    preds = np.ascontiguousarray(preds, F32)
    sc = np.ascontiguousarray(sc, F32).reshape(n, 50)
    boxes = np.ascontiguousarray(recs[:, 12:16], F32)
    bsc = np.ascontiguousarray(recs[:, 5], F32)
    pick = np.zeros(n, np.int32); pose = np.zeros((n, 50, 2), F32); score = np.zeros((n, 50), F32); prop = np.zeros(n, F32)
    m = _lib.lib().bp_pose_nms(boxes.ctypes.data, bsc.ctypes.data, preds.ctypes.data, sc.ctypes.data, n, 50, pick.ctypes.data,
                               pose.ctypes.data, score.ctypes.data, prop.ctypes.data)
    assert m >= 0
    s = np.where(sc == 0, F32(1e-5), sc)
    ref_d = (F32(0.1) * np.maximum(boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1])).astype(F32)
    human = np.array([np.cumsum(s[i], dtype=F32)[-1] / F32(50) for i in range(n)], F32)
    ids = list(range(n))
    picks, clusters, g_simi, g_dist = [], [], np.inf, np.inf
    while ids and n > 1:
        ref = ids[int(np.argmax(human[ids]))]
        dele = []
        for c in ids:
            d = np.sqrt(((preds[ref] - preds[c]) ** 2).sum(1, dtype=F32)).astype(F32)
            simi = (np.tanh(s[ref]) * np.tanh(s[c]))[d <= 1].sum(dtype=F32) + F32(1.7) * np.exp(-d / F32(2.65)).sum(dtype=F32)
            nmatch = int((d / min(ref_d[ref], F32(7)) <= 1).sum())
            g_simi = min(g_simi, abs(float(simi) - 22.48))
            for lim in (1.0, float(min(ref_d[ref], 7)), float(min(ref_d[ref], 15))):
                g_dist = min(g_dist, float(np.abs(d - F32(lim)).min()))
            if simi > 22.48 or nmatch >= 5:
                dele.append(c)
        if not dele:
            dele = [ref]
        picks.append(ref); clusters.append(sum(1 << c for c in dele))
        ids = [c for c in ids if c not in dele]
    if n == 1:
        picks, clusters = [0], [1]
    masks = [clusters[picks.index(int(pick[j]))] for j in range(m)]
    return m, pick, pose, score, prop, masks, g_simi, g_dist


@pytest.mark.parametrize("left", [50, 10])
def test_candidate_tail_matches_host(cuda, left):
    cases = _cases()
    Cmax = 8
    recs = np.zeros((len(cases) + 1, Cmax, 316), F32)
    recs[:, :, 0] = np.array([-1], np.int32).view(F32)[0]
    counts = np.zeros(len(cases) + 1, np.int32)                       # the last frame: count 0
    for i, (_, r) in enumerate(cases):
        recs[i, :len(r)] = r
        counts[i] = len(r)
    poses, merged, info = ops.pose_from_candidate_records(torch.from_numpy(recs).to(cuda), torch.from_numpy(counts).to(cuda),
                                                          KP3D, CAM_K, left)
    poses, merged, info = poses.cpu().numpy(), merged.cpu().numpy(), info.cpu().numpy()
    assert poses[-1, 0] == 1 and list(info[-1]) == [0, 0, -1, 0]
    got = finish_candidate_pose_record(recs[-1], 0, poses[-1], merged[-1], info[-1], "e.png")
    assert got == finish_candidate_records(recs[-1], 0, "e.png", KP3D, CAM_K, left)
    expect_m = {"coincident": 1, "simi": 1}
    for i, (name, r) in enumerate(cases):
        n = len(r)
        m, pick, pose, score, prop, masks, g_simi, g_dist = _host_nms(r)
        print("%-22s left %d: m %d, margin simi %.4g, distance %.4g" % (name, left, m, g_simi, g_dist))
        assert g_simi >= 1e-3 and g_dist >= 1e-4, name                # precondition: every decision has a margin
        kind = name.split()[0]
        if kind in expect_m:
            assert m == 1 and masks[0] == (1 << n) - 1, name          # everything merged into candidate 0
        elif kind in ("far", "below"):
            assert m == n and all(bin(k).count("1") == 1 for k in masks), name
        elif name == "two clusters":
            assert m == 2 and sorted(masks) == [0b00111, 0b11000]
        elif name == "first pick filtered":
            assert m == 1 and pick[0] == 1
        assert list(info[i]) == [n, m, 0 if m else -1, masks[0] if m else 0], name
        for j in range(m):
            assert int(merged[i, j, :1].view(np.int32)[0]) == int(pick[j]), name
            np.testing.assert_array_equal(_bits(merged[i, j, 1:2]), _bits(prop[j:j + 1]), err_msg=name)
            mg = merged[i, j, 2:].reshape(50, 3)
            np.testing.assert_array_equal(_bits(mg[:, :2]), _bits(pose[j]), err_msg=name)
            np.testing.assert_array_equal(_bits(mg[:, 2]), _bits(score[j]), err_msg=name)
        want = finish_candidate_records(r, n, "c.png", KP3D, CAM_K, left)
        got = finish_candidate_pose_record(recs[i], n, poses[i], merged[i], info[i], "c.png")
        assert poses[i, 0] == 0 and int(poses[i, 1]) == min(50, left), name
        np.testing.assert_array_equal(_bits(poses[i, 16:].astype(F32).reshape(50, 3)[:, :2]), _bits(want["result"][0]["keypoints"]))
        np.testing.assert_array_equal(_bits(poses[i, 14:15].astype(F32)), _bits(want["result"][0]["proposal_score"]))
        assert got.keys() == want.keys()
        assert len(got["result"]) == len(want["result"]) == m
        for a, b in zip(got["result"], want["result"]):
            for k in b:
                np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg="%s %s" % (name, k))
        for k in ("boxes", "scores", "yolo_indices"):
            np.testing.assert_array_equal(got[k], want[k])
        d = max(np.abs(got["cam_R"] - want["cam_R"]).max(), np.abs(got["cam_t"] - want["cam_t"]).max())
        print("%-22s left %d: |R, t| difference %.3g" % (name, left, d))
        assert d <= RT_TOL, (name, d)


# ------------------------------------------------------------------ harness
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _evaluate(outdir, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--synthetic", "4", "--sp", "--outdir", str(outdir)] + list(flags),
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(os.path.join(str(outdir), "Betapose-results.json")).read()


def test_evaluate_candidates(tmp_path):
    """evaluate.py --synthetic 4 --candidates 3 --sp writes the same JSON with and without --device_pnp (key points and
    scores equal, R and t to the tail's bar); --candidates 1 writes the fused harness' JSON byte for byte."""
    host = json.loads(_evaluate(tmp_path / "host", "--candidates", "3"))
    dev = json.loads(_evaluate(tmp_path / "dev", "--candidates", "3", "--device_pnp"))
    assert len(host) == len(dev) > 0
    for x, y in zip(host, dev):
        assert x["image_id"] == y["image_id"] and x["keypoints"] == y["keypoints"] and x["score"] == y["score"]
        d = max(np.abs(np.subtract(x["cam_R"], y["cam_R"])).max(), np.abs(np.subtract(x["cam_t"], y["cam_t"])).max())
        print("%s: |R, t| difference host / device tail %.3g" % (x["image_id"], d))
        assert d <= RT_TOL
    assert _evaluate(tmp_path / "one", "--candidates", "1") == _evaluate(tmp_path / "fused", "--fused")


def test_evaluate_candidates_refuses_ransac_and_shared_detector(tmp_path):
    for script, flags, word in (("evaluate.py", ["--pnp_ransac"], "--pnp_ransac"),
                                ("occlusion_evaluate.py", ["--pnp_ransac"], "--pnp_ransac"),
                                ("occlusion_evaluate.py", ["--shared_detector", "x.cfg"], "--shared_detector")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--synthetic", "2", "--outdir", str(tmp_path), "--candidates", "3"] + flags,
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode != 0 and "--candidates cannot be combined with " + word in r.stderr, r.stderr
