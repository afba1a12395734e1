"""bench.py on the host: the --dump-outputs writer fed with the golden pipeline records (tests/golden/pipeline.npz) run
through finish_record as in a timed step, and the options a plain run refuses.  CPU only."""
import os
import subprocess
import sys

import numpy as np

import helpers
from betapose_amd import synth
from betapose_amd.pipeline import finish_record

sys.path.insert(0, helpers.ROOT)
import bench  # noqa: E402

NAMES = {"records", "boxes", "box_scores", "keypoints", "kp_scores", "proposal_scores", "cam_R", "cam_t"}


def _records(pipe):
    n = int(pipe["n_frames"])
    recs = np.zeros((n + 1, 316), np.float32)
    for i in range(n):
        k = "f%d_" % i
        recs[i, 0] = np.array([pipe[k + "obj_argmax"]], np.int32).view(np.float32)[0]
        recs[i, 5] = pipe[k + "scores"][0, 0]
        recs[i, 8:10], recs[i, 10:12], recs[i, 12:16] = pipe[k + "pt1"][0], pipe[k + "pt2"][0], pipe[k + "boxes"][0]
        kp = recs[i, 16:].reshape(50, 6)
        kp[:, 0] = pipe[k + "kp_idx"].astype(np.int32).view(np.float32)
        kp[:, 1] = pipe[k + "kp_max"]
        kp[:, 2:] = pipe[k + "kp_nb"]
    recs[n, 0] = np.array([-1], np.int32).view(np.float32)[0]        # a frame without a detection
    return recs


def test_dump_outputs_hold_what_the_caller_received(tmp_path):
    pipe = helpers.golden("pipeline.npz")
    recs = _records(pipe)
    outs = [finish_record(r, "%06d.png" % i, synth.synth_kp3d(50), synth.CAM_K) for i, r in enumerate(recs)]
    bench.dump_outputs(str(tmp_path), recs, outs)
    got = {f[:-len(".npy")]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == NAMES
    assert all(v.dtype in (np.float32, np.float64) and len(v) == len(recs) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    for i in range(int(pipe["n_frames"])):
        k = "f%d_" % i
        # int32 fields as their values, not their bits
        assert got["records"][i, 0] == int(pipe[k + "obj_argmax"])
        np.testing.assert_array_equal(got["records"][i, 16::6], pipe[k + "kp_idx"])
        np.testing.assert_array_equal(got["records"][i, 17::6], pipe[k + "kp_max"])
        np.testing.assert_array_equal(got["records"][i, 8:16], recs[i, 8:16])
        np.testing.assert_array_equal(got["boxes"][i], pipe[k + "boxes"][0])
        np.testing.assert_allclose(got["keypoints"][i], pipe[k + "nms_kp"], rtol=1e-6, atol=2e-5)
        np.testing.assert_allclose(got["kp_scores"][i], pipe[k + "nms_score"][:, 0], rtol=1e-6)
        np.testing.assert_array_equal(got["cam_R"][i], np.asarray(outs[i]["cam_R"]))
        np.testing.assert_array_equal(got["cam_t"][i], np.asarray(outs[i]["cam_t"]).reshape(3))
    assert got["records"][-1, 0] == -1
    for name in NAMES - {"records"}:
        assert np.isnan(got[name][-1]).all(), name


def test_plain_run_refuses_what_needs_full():
    for extra in (["--repeats", "3"], ["--insitu", "layers.txt"], ["--steps", "0"]):
        r = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py")] + extra, capture_output=True, text=True,
                           timeout=120, cwd=helpers.ROOT)
        assert r.returncode == 2 and "error" in r.stderr, (extra, r.stderr[-2000:])
        assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
