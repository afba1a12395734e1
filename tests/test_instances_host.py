"""A pose for every merged candidate, host side: ``pipeline.finish_candidate_records(all_instances=True)``, the JSON
writer's per-entry poses and ``metrics.evaluate_results(match_instances=True)``.  No GPU: the host solver and pose NMS
behind the C ABI are plain C++."""
import json

import numpy as np
import pytest

import instances_common as ic
import test_gpu_candidates as tc
from test_gpu_pose_tail import _one_ulp_sensitivity
from betapose_amd import _lib, metrics, ops
from betapose_amd.eval import decode_keypoints
from betapose_amd.pipeline import finish_candidate_records
from betapose_amd.pPose_nms import pose_nms, results_to_json_list
from betapose_amd.synth import CAM_K

KP3D = ic.KP3D
F32 = np.float32


def _same(a, b):
    """Equality of two result dicts' values, arrays by bits."""
    if isinstance(b, dict):
        assert isinstance(a, dict) and a.keys() == b.keys()
        for k in b:
            _same(a[k], b[k])
    elif isinstance(b, list):
        assert isinstance(a, list) and len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(b, np.ndarray):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
        assert a.tobytes() == b.tobytes()
    else:
        assert a == b and type(a) is type(b)


def _todays_dict(r, n, name, left):
    """``finish_candidate_records`` as it stood before instances, restated from its parts (n >= 2)."""
    idx = r[:, :1].copy().view(np.int32)[:, 0]
    boxes, scores = r[:, 12:16].copy(), r[:, 5:6].copy()
    _, preds, sc = decode_keypoints(r[:, 16:].reshape(n, 50, 6), r[:, 8:10], r[:, 10:12])
    result = pose_nms(boxes, scores, preds, sc)
    out = {"imgname": name, "result": result, "boxes": boxes, "scores": scores, "yolo_index": int(idx[0]), "yolo_indices": idx}
    if result:
        R, t = ic.host_instance_pose(result[0], left)
        out.update({"cam_R": R, "cam_t": t})
    else:
        out.update({"cam_R": [], "cam_t": []})
    return out


@pytest.mark.parametrize("left", [50, 10])
def test_without_the_flag_the_dict_is_unchanged(left):
    """(guard)"""
    for name, r in ic.cases():
        n = len(r)
        got = finish_candidate_records(r, n, "c.png", KP3D, CAM_K, left)
        assert "instances" not in got
        if n == 0:
            assert got == {"imgname": "c.png", "result": [], "cam_R": [], "cam_t": [], "boxes": None}
        else:
            _same(got, _todays_dict(r, n, "c.png", left))
        _same(finish_candidate_records(r, n, "c.png", KP3D, CAM_K, left, all_instances=False), got)


@pytest.mark.parametrize("left", [50, 10])
def test_instances_parallel_to_result(left):
    seen_m = set()
    for name, r in ic.cases():
        n = len(r)
        plain = finish_candidate_records(r, n, "c.png", KP3D, CAM_K, left)
        got = finish_candidate_records(r, n, "c.png", KP3D, CAM_K, left, all_instances=True)
        inst = got.pop("instances")
        _same(got, plain)                                            # everything else is today's dict
        assert len(inst) == len(plain["result"]), name
        if n == 0:
            assert inst == []
            continue
        m, pick, _, _, _, _, _, _ = tc._host_nms(r)
        assert m == len(inst), name
        seen_m.add(m)
        for j, s in enumerate(inst):
            assert set(s) == {"cam_R", "cam_t", "status", "points", "pick", "bbox"}
            assert s["pick"] == int(pick[j]) and s["status"] == 0 and s["points"] == min(50, left), (name, j)
            np.testing.assert_array_equal(s["bbox"], r[int(pick[j]), 12:16])
            np.testing.assert_array_equal(plain["result"][j]["bbox"], r[0, 12:16])      # pPose_nms.py:116
            if j == 0:
                assert s["cam_R"].tobytes() == plain["cam_R"].tobytes() and s["cam_t"].tobytes() == plain["cam_t"].tobytes()
            else:
                R, t = ic.host_instance_pose(plain["result"][j], left)
                assert s["cam_R"].tobytes() == R.tobytes() and s["cam_t"].tobytes() == t.tobytes(), (name, j)
    assert {0, 1, 2, 3, 8} <= seen_m


def test_count_one_and_count_zero():
    rec = tc._base_record(np.random.default_rng(3), scores=(0.8, 0.95))[None]
    one = finish_candidate_records(rec, 1, "a.png", KP3D, CAM_K, 50, all_instances=True)
    assert len(one["instances"]) == len(one["result"]) == 1
    s = one["instances"][0]
    assert s["pick"] == 0 and s["status"] == 0 and s["points"] == 50
    assert s["cam_R"].tobytes() == one["cam_R"].tobytes() and s["cam_t"].tobytes() == one["cam_t"].tobytes()
    np.testing.assert_array_equal(s["bbox"], rec[0, 12:16])
    plain = finish_candidate_records(rec, 1, "a.png", KP3D, CAM_K, 50)
    assert "instances" not in plain
    one.pop("instances")
    _same(one, plain)
    assert finish_candidate_records(rec, 0, "a.png", KP3D, CAM_K, 50, all_instances=True)["instances"] == []


def test_failed_instance_is_recorded_and_first_is_raised(monkeypatch):
    """With 3 key points left every PnP fails: result[0]'s failure raises, as without the flag.  A failure of an instance
    j > 0 alone (the solver's status stubbed for it) is recorded with the solver's code."""
    from betapose_amd import pipeline
    r = dict(ic.cases())["rigid n=2"]
    for flag in (False, True):
        with pytest.raises(_lib.BetaposeHipError):
            finish_candidate_records(r, 2, "a.png", KP3D, CAM_K, 3, all_instances=flag)
    assert ops.solve_pnp_status(KP3D[:3], np.zeros((3, 2)), CAM_K)[2] < 0
    assert ops.solve_pnp_status(KP3D[:3], np.zeros((3, 2)), CAM_K)[:2] == ([], [])
    monkeypatch.setattr(pipeline, "solve_pnp_status", lambda *a: ([], [], -2))
    got = finish_candidate_records(r, 2, "a.png", KP3D, CAM_K, 50, all_instances=True)
    assert got["instances"][0]["status"] == 0 and len(got["instances"][0]["cam_R"]) == 3
    s = got["instances"][1]
    assert s["status"] == -2 and s["cam_R"] == [] and s["cam_t"] == [] and s["pick"] == 1 and s["points"] == 50


def test_planted_instances_are_well_conditioned():
    """The precondition of the GPU test's host bar: the host solver's own one-ulp movement of every planted instance
    j > 0 stays below RT_TOL / 10, except on the frames instances_common.HOST_BAR_EXCLUDED names."""
    for left in (50, 10):
        for name, r in ic.cases():
            if len(r) < 2 or (name, left) in ic.HOST_BAR_EXCLUDED:
                continue
            d = finish_candidate_records(r, len(r), "a.png", KP3D, CAM_K, left)
            for j in range(1, len(d["result"])):
                k3, k2 = ic.pruned_points(d["result"][j]["keypoints"], d["result"][j]["kp_score"], left)
                sens = _one_ulp_sensitivity(k3, k2, 1.0)
                assert sens < ic.RT_TOL / 10, (name, left, j, sens)


def test_json_entries_carry_their_own_pose():
    cs = dict(ic.cases())
    frames = [("0003.png", cs["rigid n=3"]), ("0004.png", cs["two clusters"]), ("0005.png", cs["coincident n=2"])]
    plain = [finish_candidate_records(r, len(r), nm, KP3D, CAM_K, 50) for nm, r in frames]
    full = [finish_candidate_records(r, len(r), nm, KP3D, CAM_K, 50, all_instances=True) for nm, r in frames]
    for for_eval in (False, True):
        want = results_to_json_list(plain, for_eval)
        got = results_to_json_list(full, for_eval)
        assert len(got) == len(want) == 3 + 2 + 1
        k = 0
        for f in full:
            for j, s in enumerate(f["instances"]):
                assert got[k]["cam_R"] == s["cam_R"].reshape(9).tolist() and got[k]["cam_t"] == s["cam_t"].reshape(3).tolist()
                assert {x: got[k][x] for x in got[k] if x not in ("cam_R", "cam_t")} == \
                       {x: want[k][x] for x in want[k] if x not in ("cam_R", "cam_t")}
                if j > 0:
                    assert got[k]["cam_R"] != want[k]["cam_R"]       # today: result[0]'s pose stamped on every entry
                k += 1
        # without the key: byte for byte what it is today (every entry carries the frame's pose)
        stripped = [{k_: v for k_, v in f.items() if k_ != "instances"} for f in full]
        assert json.dumps(results_to_json_list(stripped, for_eval)) == json.dumps(want)
        k = 0
        for f in plain:
            for _ in f["result"]:
                assert want[k]["cam_R"] == f["cam_R"].reshape(9).tolist()
                k += 1
    # a failed instance: its entry has no pose, the others keep theirs
    full[0]["instances"][1].update({"cam_R": [], "cam_t": [], "status": -2})
    got = results_to_json_list(full)
    assert "cam_R" not in got[1] and "cam_t" not in got[1] and "cam_R" in got[0] and "cam_R" in got[2]


# ------------------------------------------------------------------ scoring
def _pose(rotvec, t):
    from scipy.spatial.transform import Rotation as Rot
    P = np.eye(4)
    P[:3, :3] = Rot.from_rotvec(rotvec).as_matrix()
    P[:3, 3] = t
    return P


def _two_instance_frame():
    A, B = _pose([0.3, -0.5, 0.2], [0.02, -0.03, 0.8]), _pose([-0.2, 0.4, 0.1], [-0.2, 0.05, 0.9])
    box_a, box_b = np.array([300.0, 200.0, 400.0, 320.0], F32), np.array([100.0, 180.0, 190.0, 290.0], F32)
    kp = {"keypoints": np.zeros((50, 2), F32), "kp_score": np.ones((50, 1), F32), "proposal_score": np.ones(1, F32)}
    frame = {"imgname": "0007.png", "boxes": np.array([box_a, box_b]),
             "result": [dict(kp, bbox=box_a.copy()), dict(kp, bbox=box_a.copy())],       # pPose_nms.py:116: always the first box
             "cam_R": A[:3, :3].copy(), "cam_t": A[:3, 3:].copy(),
             "instances": [{"cam_R": A[:3, :3].copy(), "cam_t": A[:3, 3:].copy(), "status": 0, "points": 50, "pick": 0, "bbox": box_a},
                           {"cam_R": B[:3, :3].copy(), "cam_t": B[:3, 3:].copy(), "status": 0, "points": 50, "pick": 1, "bbox": box_b}]}
    xywh = lambda b: [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])]  # noqa: E731
    gt = {7: [{"pose": B, "bbox": xywh(box_b)}, {"pose": A, "bbox": xywh(box_a)}]}        # the opposite order
    return frame, gt


def test_evaluate_results_matches_instances_by_box():
    frame, gt = _two_instance_frame()
    model = np.random.default_rng(4).uniform(-0.05, 0.05, (200, 3))
    args = (gt, model, CAM_K, 100.0)
    m = metrics.evaluate_results([frame], *args, match_instances=True)
    assert m["n"] == 2 and m["mean_iou"] == 1.0 and m["mean_add"] == 1.0 and m["mean_2d_acc"] == 1.0
    assert m["mean_add_err_mm"] == 0.0                               # both matched to their own pose
    # today's numbers: every annotation against result[0] -- with or without the key, and by default
    stripped = {k: v for k, v in frame.items() if k != "instances"}
    today = metrics.evaluate_results([stripped], *args)
    assert metrics.evaluate_results([frame], *args, match_instances=False) == today
    assert metrics.evaluate_results([frame], *args) == today
    assert metrics.evaluate_results([stripped], *args, match_instances=True) == today    # no instances: today's rule
    assert today["n"] == 2 and today["mean_iou"] == 0.5 and today["mean_add_err_mm"] == 0.0
    # one instance deleted: one hit, one miss
    for drop, in ((0,), (1,)):
        f = dict(frame, instances=[s for j, s in enumerate(frame["instances"]) if j != drop])
        m = metrics.evaluate_results([f], *args, match_instances=True)
        assert m["n"] == 2 and m["mean_iou"] == 0.5 and m["mean_add"] == 1.0 and m["mean_add_err_mm"] == 0.0
    # an instance whose PnP failed is no candidate for a match
    f = dict(frame, instances=[frame["instances"][0], dict(frame["instances"][1], cam_R=[], cam_t=[], status=-2)])
    m = metrics.evaluate_results([f], *args, match_instances=True)
    assert m["n"] == 2 and m["mean_iou"] == 0.5
    # swapped poses: the match is by box, so both pairs now carry the other instance's pose
    sw = dict(frame, instances=[dict(frame["instances"][0], bbox=frame["instances"][1]["bbox"]),
                                dict(frame["instances"][1], bbox=frame["instances"][0]["bbox"])])
    m = metrics.evaluate_results([sw], *args, match_instances=True)
    assert m["n"] == 2 and m["mean_iou"] == 1.0 and m["mean_add_err_mm"] > 50.0


def test_evaluate_results_ties_go_to_the_lower_instance():
    frame, gt = _two_instance_frame()
    box = frame["instances"][0]["bbox"]
    tie = dict(frame, instances=[dict(frame["instances"][0]), dict(frame["instances"][1], bbox=box)])
    gt1 = {7: [gt[7][1]]}                                            # annotation A alone; both instances sit on its box
    m = metrics.evaluate_results([tie], gt1, np.eye(3), CAM_K, 100.0, match_instances=True)
    assert m["n"] == 1 and m["mean_add_err_mm"] == 0.0               # instance 0 (pose A), not instance 1 (pose B)
