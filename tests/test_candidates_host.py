"""Candidate boxes per frame, host side: the numpy restatement of the reference's live-NMS branch (tests/nms_ref.py) is
pinned to the oracle's ``write_results``, and ``pipeline.finish_candidate_records`` is pinned to ``finish_record`` (one
candidate) and to the reference's ``pose_nms`` fixtures (several)."""
import numpy as np
import torch

import helpers
import nms_ref
from betapose_amd import pipeline
from betapose_amd.synth import CAM_K, synth_kp3d

KP3D = synth_kp3d(50)


def test_nms_ref_candidate0_is_write_results_row():
    """On every prediction tensor of the golden set, candidate 0 of the restatement is the row the reference keeps."""
    from oracle import yolo_ref
    e = helpers.golden("edges.npz")
    n_rows = 0
    for t in range(int(e["sel_n"])):
        pred = e["sel%d_pred" % t]
        conf = float(e["sel%d_conf" % t])
        want = yolo_ref.write_results(torch.from_numpy(pred).clone(), conf, 80)
        for C in (1, 3):
            recs, counts = nms_ref.select_nms(pred, conf, 80, 0.4, C)
            have = np.nonzero(counts > 0)[0]
            if isinstance(want, int):
                assert want == 0 and have.size == 0, t
                continue
            w = want.numpy()
            assert list(w[:, 0].astype(int)) == list(have), t
            for row, b in zip(w, have):
                np.testing.assert_array_equal(recs[b, 0, 1:], row[1:].astype(np.float32), err_msg="case %d image %d" % (t, b))
                # the row kept is the first row of highest objectness among the live rows of class 0
                p = pred[b]
                live = (p[:, 4] > np.float32(conf)) & (np.argmax(p[:, 5:5 + min(80, p.shape[1] - 5)], axis=1) == 0)
                obj = np.where(live, p[:, 4], -1.0)
                assert int(recs[b, 0, :1].view(np.int32)[0]) == int(np.argmax(obj))
                n_rows += 1
            assert (counts <= C).all()
    assert n_rows > 40


def _record_from_golden(pipe, k):
    """The 316-float record the device pipeline would write for golden frame k (tests/golden/pipeline.npz)."""
    rec = np.zeros(316, np.float32)
    rec[0] = np.array([int(pipe[k + "obj_argmax"])], np.int32).view(np.float32)[0]
    rec[5] = pipe[k + "scores"][0, 0]
    rec[8:10], rec[10:12] = pipe[k + "pt1"][0], pipe[k + "pt2"][0]
    rec[12:16] = pipe[k + "boxes"][0]
    kp = rec[16:].reshape(50, 6)
    kp[:, 0] = pipe[k + "kp_idx"].astype(np.int32).view(np.float32)
    kp[:, 1] = pipe[k + "kp_max"]
    return rec


def test_one_candidate_is_finish_record():
    pipe = helpers.golden("pipeline.npz")
    for i in range(int(pipe["n_frames"])):
        k = "f%d_" % i
        if k + "kp_idx" not in pipe.files:
            rec = np.zeros(316, np.float32)
            rec[0] = np.array([7], np.int32).view(np.float32)[0]
            rec[5] = 0.8
            rec[8:12] = [100, 80, 300, 330]
            rec[12:16] = [120, 100, 280, 310]
            rng = np.random.default_rng(i)
            kp = rec[16:].reshape(50, 6)
            kp[:, 0] = rng.integers(65, 78 * 64, 50).astype(np.int32).view(np.float32)
            kp[:, 1] = rng.uniform(0.35, 0.9, 50)
            kp[:, 2:] = rng.uniform(0, 0.3, (50, 4))
        else:
            rec = _record_from_golden(pipe, k)
        for left in (50, 10):
            want = pipeline.finish_record(rec, "%d.png" % i, KP3D, CAM_K, left)
            rows = np.zeros((3, 316), np.float32)
            rows[0] = rec
            rows[1:, 0] = np.array([-1], np.int32).view(np.float32)[0]
            got = pipeline.finish_candidate_records(rows, 1, "%d.png" % i, KP3D, CAM_K, left)
            assert got.keys() == want.keys()
            for f in want:
                if f == "result":
                    assert len(got[f]) == len(want[f]) == 1
                    for key in want[f][0]:
                        np.testing.assert_array_equal(got[f][0][key], want[f][0][key])
                elif isinstance(want[f], np.ndarray):
                    np.testing.assert_array_equal(got[f], want[f])
                else:
                    assert got[f] == want[f]
    none = pipeline.finish_candidate_records(np.zeros((2, 316), np.float32), 0, "x.png", KP3D, CAM_K)
    assert none == {"imgname": "x.png", "result": [], "cam_R": [], "cam_t": [], "boxes": None}


def test_several_candidates_forward_to_pose_nms(monkeypatch):
    """On the 24 golden pose-NMS sets ``finish_candidate_records`` hands pose_nms the n decoded candidates unchanged: its
    'result' is the fixture's."""
    g = helpers.golden("edges.npz")
    seen = 0
    for t in range(int(g["nms_n"])):
        boxes, bsc = g["nms%d_boxes" % t], g["nms%d_bsc" % t]
        poses, psc = g["nms%d_poses" % t], g["nms%d_psc" % t]
        n = len(boxes)
        recs = np.zeros((n, 316), np.float32)
        recs[:, 0] = np.arange(n).astype(np.int32).view(np.float32)
        recs[:, 5] = np.asarray(bsc).reshape(n)
        recs[:, 12:16] = boxes
        # the decode is not what this test is about: hand the fixture's poses through it
        monkeypatch.setattr(pipeline, "decode_keypoints", lambda kp, pt1, pt2, p=poses, s=psc: (None, p.copy(), s.copy()))
        out = pipeline.finish_candidate_records(recs, n, "s.png", KP3D, CAM_K)
        res = out["result"]
        assert len(res) == int(g["nms%d_n" % t]), t
        for j, r in enumerate(res):
            np.testing.assert_allclose(r["keypoints"], g["nms%d_o%d_kp" % (t, j)], atol=2e-4, rtol=0)
            np.testing.assert_allclose(r["kp_score"], g["nms%d_o%d_score" % (t, j)], atol=2e-6, rtol=0)
            assert abs(float(r["proposal_score"][0]) - float(g["nms%d_o%d_prop" % (t, j)])) < 1e-5
            np.testing.assert_allclose(r["bbox"], g["nms%d_o%d_bbox" % (t, j)], atol=1e-5, rtol=0)
        seen += 1
    assert seen == 24
