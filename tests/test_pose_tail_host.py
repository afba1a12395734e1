"""Host side of the device pose tail (no GPU): the C header's pose record and entry points, and
``pipeline.finish_pose_record`` turning pose rows into exactly the dicts ``finish_record`` builds."""
import os
import re

import numpy as np
import pytest

import helpers
from betapose_amd import _lib
from betapose_amd.pipeline import POSE_DOUBLES, finish_pose_record, finish_record
from betapose_amd.pPose_nms import write_json
from betapose_amd.synth import CAM_K, synth_kp3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP3D = synth_kp3d(50)


def test_header_declares_the_pose_record_and_entry_points():
    code = helpers.header_code()
    assert re.search(r"#define BP_POSE_DOUBLES 166\b", code)
    assert POSE_DOUBLES == _lib.POSE_DOUBLES == 166
    for name in ("bp_pipeline_set_pose_solver", "bp_pipeline_poses", "bp_pose_from_records", "bp_solve_pnp_batch"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.PROTOTYPES


def _record(seed, det=True, low=False):
    rng = np.random.default_rng(seed)
    rec = np.zeros(316, np.float32)
    rec[0] = np.array([3 if det else -1], np.int32).view(np.float32)[0]
    rec[5] = 0.75
    rec[8:12] = [200.0, 120.0, 420.0, 400.0]
    rec[12:16] = [210.0, 130.0, 410.0, 390.0]
    kp = rec[16:].reshape(50, 6)
    kp[:, 0] = rng.integers(0, 80 * 64, 50).astype(np.int32).view(np.float32)
    kp[:, 1] = rng.uniform(0.05, 0.29, 50) if low else rng.uniform(0.3, 0.95, 50)
    kp[:, 2:] = rng.uniform(0, 0.3, (50, 4))
    return rec


def _row_from_host(out, status=None, used=50):
    """The pose row the device tail writes for the frame whose host dict is ``out``."""
    row = np.zeros(POSE_DOUBLES)
    row[2:14] = np.nan
    if out["boxes"] is None:
        row[0] = 1
        return row
    if not out["result"]:
        row[0] = 2
        return row
    r = out["result"][0]
    row[0] = 0 if status is None else status
    row[1] = used
    if status is None:
        row[2:11] = out["cam_R"].reshape(9)
        row[11:14] = out["cam_t"].reshape(3)
    row[14] = r["proposal_score"][0]
    row[16:] = np.concatenate([r["keypoints"], r["kp_score"]], axis=1).astype(np.float64).reshape(150)
    return row


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "result":
            assert len(a[k]) == len(b[k])
            for ra, rb in zip(a[k], b[k]):
                assert ra.keys() == rb.keys()
                for kk in ra:
                    assert ra[kk].dtype == rb[kk].dtype and ra[kk].shape == rb[kk].shape
                    np.testing.assert_array_equal(ra[kk], rb[kk])
        elif isinstance(a[k], np.ndarray):
            assert isinstance(b[k], np.ndarray) and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            np.testing.assert_array_equal(a[k], b[k])
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("left", [50, 10])
def test_finish_pose_record_builds_the_host_dicts(tmp_path, left):
    recs = [_record(1), _record(2, det=False), _record(3, low=True), _record(4)]
    host, dev = [], []
    for i, rec in enumerate(recs):
        name = "%04d.png" % i
        out = finish_record(rec, name, KP3D, CAM_K, left)
        got = finish_pose_record(rec, _row_from_host(out, used=min(50, left)), name)
        _assert_same(got, out)
        host.append(out)
        dev.append(got)
    assert host[0]["result"] and host[1]["boxes"] is None and host[2]["result"] == [] and host[2]["boxes"] is not None
    for name, res in (("host", host), ("dev", dev)):
        os.makedirs(tmp_path / name)
        write_json([r for r in res if r["boxes"] is not None], str(tmp_path / name), form="default")
    assert open(tmp_path / "host" / "Betapose-results.json").read() == open(tmp_path / "dev" / "Betapose-results.json").read()


def test_finish_pose_record_raises_where_the_host_raises():
    rec = _record(5)
    with pytest.raises(_lib.BetaposeHipError) as host_err:
        finish_record(rec, "a.png", KP3D, CAM_K, 4)                   # 4 non-planar points: the solver refuses
    out = finish_record(rec, "a.png", KP3D, CAM_K, 50)
    with pytest.raises(_lib.BetaposeHipError) as dev_err:
        finish_pose_record(rec, _row_from_host(out, status=-1, used=4), "a.png")
    assert str(dev_err.value) == str(host_err.value)


def test_finish_pose_record_rejects_a_row_of_another_frame():
    rec = _record(6)
    other = _row_from_host(finish_record(_record(7, det=False), "b.png", KP3D, CAM_K, 50))   # status 1
    with pytest.raises(ValueError):
        finish_pose_record(rec, other, "a.png")
