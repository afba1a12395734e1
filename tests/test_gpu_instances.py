"""A pose for every merged candidate on the GPU (csrc/pose_tail_inst.hip): the stand-alone launch against the existing
pose row, the device solver and the host dict; ``CandidatePipeline`` with instances on and off; the packed row; the harness.

Bars: row 0 is the existing pose row bit for bit; points used, proposal score and key points of every instance are
bit-identical to the host dict; R, t are bit-identical to ``ops.solve_pnp_batch`` (the same ``pnp_wave``) on the
host-pruned points, and within RT_TOL = 1e-9 of the host ``solve_pnp`` -- beyond it only under the rule of
tests/test_gpu_pose_tail.py ``_check_batch`` (within 10x the host solver's own one-ulp movement, at most max(1, N // 20) of
N instances).  The planted frames are chosen so that the rule is not what passes the test (instances_common.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers  # noqa: E402
import instances_common as ic  # noqa: E402
from test_gpu_candidates import NMS_CONF, nets  # noqa: E402,F401  (the random-weight engines fixture)
from test_gpu_pose_tail import _one_ulp_sensitivity, _write_pngs  # noqa: E402
from betapose_amd import _lib, ops, synth  # noqa: E402
from betapose_amd.pipeline import (POSE_DOUBLES, CandidatePipeline, StreamedRunner, candidate_row_floats,  # noqa: E402
                                   finish_candidate_pose_record, finish_candidate_records, unpack_candidate_row)
from betapose_amd.synth import CAM_K  # noqa: E402

KP3D = ic.KP3D
F32 = np.float32
RT_TOL = ic.RT_TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _rt_diff(R, t, hR, ht):
    return max(np.abs(np.asarray(R) - hR).max(), np.abs(np.asarray(t).reshape(3) - np.asarray(ht).reshape(3)).max())


def _hold_to_host_bar(diffs):
    """``diffs``: [(label, |R, t| difference, pruned 3-D, pruned 2-D)] of the solved instances: RT_TOL, else the rule of
    tests/test_gpu_pose_tail.py _check_batch."""
    beyond = [x for x in diffs if x[1] > RT_TOL]
    for label, d, k3, k2 in beyond:
        sens = _one_ulp_sensitivity(k3, k2, 1.0)
        assert d <= 10 * sens, (label, d, sens)
    assert len(beyond) <= max(1, len(diffs) // 20), ([x[:2] for x in beyond], len(diffs))


@pytest.fixture(scope="module")
def host_dicts():
    """The host dicts of every planted frame, computed once: {(name, left): dict}."""
    out = {}
    for left in (50, 10):
        for name, r in ic.cases() + ic.cases_for(1):
            out[(name, left)] = finish_candidate_records(r, len(r), "c.png", KP3D, CAM_K, left, all_instances=True)
    return out


@pytest.mark.parametrize("Cn", [8, 2, 1])
@pytest.mark.parametrize("left", [50, 10])
def test_instance_launch_matches_pose_row_device_solver_and_host(cuda, host_dicts, left, Cn):
    names, recs, counts = ic.pack(ic.cases_for(Cn), Cn)
    assert "no candidate" in names and (Cn < 2 or {"all filtered", "first pick filtered", "rigid n=2"} <= set(names))
    assert Cn > 1 or (counts == 1).sum() >= 4
    poses, merged, info = ops.pose_from_candidate_records(torch.from_numpy(recs).to(cuda), torch.from_numpy(counts).to(cuda),
                                                          KP3D, CAM_K, left)
    inst = ops.pose_instances(merged, info, poses, KP3D, CAM_K, left)
    assert inst.shape == (len(names), Cn, POSE_DOUBLES) and inst.dtype == torch.float64
    poses, info, inst = poses.cpu().numpy(), info.cpu().numpy(), inst.cpu().numpy()
    P3, P2, where = {}, {}, {}
    seen_m, seen_status = set(), set()
    for i, name in enumerate(names):
        want = host_dicts[(name, left)]
        m = int(info[i, 1])
        seen_m.add(m)
        seen_status.add(int(poses[i, 0]))
        np.testing.assert_array_equal(_bits64(inst[i, 0]), _bits64(poses[i]), err_msg=name)         # row 0: the existing row
        for j in range(max(m, 1), Cn):                                                              # no merged pose there
            row = inst[i, j]
            assert row[0] == 1 and np.isnan(row[2:14]).all() and not row[1:2].any() and not row[14:].any(), (name, j)
        assert m == len(want["result"]) == len(want["instances"]), name
        for j in range(1, m):
            row, hum, hin = inst[i, j], want["result"][j], want["instances"][j]
            assert int(row[1]) == hin["points"] == min(50, left) and row[15] == 0, (name, j)
            np.testing.assert_array_equal(_bits(row[14:15].astype(F32)), _bits(hum["proposal_score"]), err_msg=name)
            kp = row[16:].reshape(50, 3)
            assert np.array_equal(kp, kp.astype(F32))                                              # f32 values, exactly
            np.testing.assert_array_equal(_bits(kp[:, :2]), _bits(hum["keypoints"]), err_msg=name)
            np.testing.assert_array_equal(_bits(kp[:, 2:]), _bits(hum["kp_score"]), err_msg=name)
            k3, k2 = ic.pruned_points(hum["keypoints"], hum["kp_score"], left)
            P3.setdefault(len(k2), []).append(k3)
            P2.setdefault(len(k2), []).append(k2)
            where.setdefault(len(k2), []).append((i, j, name))
    if Cn == 8:
        assert {0, 1, 2, 3, 8} <= seen_m and {0, 1, 2} <= seen_status
    # R, t: the device solver on the host-pruned points, bit for bit; the host solver to its bar
    diffs = []
    for npts in P3:
        R, t, st = ops.solve_pnp_batch(np.array(P3[npts]), np.array(P2[npts]), CAM_K)
        R, t, st = R.cpu().numpy(), t.cpu().numpy(), st.cpu().numpy()
        for p, (i, j, name) in enumerate(where[npts]):
            row, hin = inst[i, j], host_dicts[(name, left)]["instances"][j]
            assert int(row[0]) == int(st[p]) == hin["status"] == 0, (name, j, row[0], st[p])
            np.testing.assert_array_equal(_bits64(row[2:11]), _bits64(R[p].reshape(9)), err_msg="%s j=%d R" % (name, j))
            np.testing.assert_array_equal(_bits64(row[11:14]), _bits64(t[p].reshape(3)), err_msg="%s j=%d t" % (name, j))
            d = _rt_diff(row[2:11].reshape(3, 3), row[11:14], hin["cam_R"], hin["cam_t"])
            held = (name, left) not in ic.HOST_BAR_EXCLUDED
            print("%-22s C %d left %d j %d: |R, t| difference to the host %.3g%s" % (name, Cn, left, j, d, "" if held else "  (not held: ill-conditioned)"))
            if held:
                diffs.append(("%s j=%d" % (name, j), d, P3[npts][p], P2[npts][p]))
    if Cn > 1:
        assert len(diffs) > 0
        _hold_to_host_bar(diffs)
    # the device dict from the rows = the host dict
    for i, name in enumerate(names):
        want = host_dicts[(name, left)]
        got = finish_candidate_pose_record(recs[i], int(counts[i]), poses[i], merged[i].cpu().numpy(), info[i], "c.png",
                                           inst_poses=inst[i])
        _same_dict(got, want, name, (name, left) not in ic.HOST_BAR_EXCLUDED)


def _same_dict(got, want, name, held=True):
    assert got.keys() == want.keys(), name
    assert len(got["instances"]) == len(want["instances"]) == len(got["result"]) == len(want["result"]), name
    for a, b in zip(got["result"], want["result"]):
        for k in b:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg="%s %s" % (name, k))
    diffs = []
    for j, (a, b) in enumerate(zip(got["instances"], want["instances"])):
        assert a.keys() == b.keys()
        assert (a["status"], a["points"], a["pick"]) == (b["status"], b["points"], b["pick"]), (name, j)
        np.testing.assert_array_equal(_bits(a["bbox"]), _bits(b["bbox"]))
        assert (len(a["cam_R"]) > 0) == (len(b["cam_R"]) > 0)
        if len(b["cam_R"]) and held:
            k3, k2 = ic.pruned_points(want["result"][j]["keypoints"], want["result"][j]["kp_score"], b["points"])
            diffs.append(("%s j=%d" % (name, j), _rt_diff(a["cam_R"], a["cam_t"], b["cam_R"], b["cam_t"]), k3, k2))
    if diffs:
        assert got["instances"][0]["cam_R"] is got["cam_R"] or np.array_equal(got["instances"][0]["cam_R"], got["cam_R"])
    return diffs


def test_instance_launch_is_deterministic_across_streams(cuda):
    names, recs, counts = ic.pack(ic.cases_for(8), 8)
    poses, merged, info = ops.pose_from_candidate_records(torch.from_numpy(recs).to(cuda), torch.from_numpy(counts).to(cuda),
                                                          KP3D, CAM_K, 50)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            outs.append(ops.pose_instances(merged, info, poses, KP3D, CAM_K, 50))
        st.synchronize()
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))


def test_instance_argument_errors(nets, cuda):
    for Cn in (0, 9):
        with pytest.raises(_lib.BetaposeHipError):
            ops.pose_instances(torch.zeros((1, Cn, 152), device=cuda), torch.zeros((1, 4), dtype=torch.int32, device=cuda),
                               torch.zeros((1, 166), dtype=torch.float64, device=cuda), KP3D, CAM_K, 50)
    det, pose = nets
    cp = CandidatePipeline(det, pose, 480, 640, candidates=3, nms_conf=NMS_CONF)
    L = _lib.lib()
    assert L.bp_cands_instance_poses(cp._h) is None
    with pytest.raises(_lib.BetaposeHipError):                       # no solver set
        _lib.check(L.bp_cands_set_instance_poses(cp._h, 1, None))
    cp.set_pose_solver(KP3D, CAM_K, 50)
    assert cp.inst_poses is None and L.bp_cands_instance_poses(cp._h) is None
    _lib.check(L.bp_cands_set_instance_poses(cp._h, 1, None))        # the object's own buffer
    assert L.bp_cands_instance_poses(cp._h) is not None
    _lib.check(L.bp_cands_set_instance_poses(cp._h, 0, None))
    assert L.bp_cands_instance_poses(cp._h) is None


def _state(cp):
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in (cp.results, cp.counts, cp.poses, cp.merged, cp.info)]


def test_candidate_pipeline_with_instances(nets, cuda):
    det, pose = nets
    frame = helpers.frames(1)[0]
    mk = lambda graph=True: CandidatePipeline(det, pose, 480, 640, candidates=3, nms_conf=NMS_CONF, use_graph=graph)  # noqa: E731
    base = mk().set_pose_solver(KP3D, CAM_K, 50).prepare()           # never saw the new argument
    n0 = base.kernel_count()
    rows, n = base.run(frame)
    want = _state(base)
    on = mk().set_pose_solver(KP3D, CAM_K, 50, all_instances=True).prepare()
    assert on.kernel_count() == n0 + 1
    assert tuple(on.inst_poses.shape) == (3, POSE_DOUBLES)
    # (guard) switched off again: the count and every output are those of the pipeline that never had it
    off = mk().set_pose_solver(KP3D, CAM_K, 50, all_instances=True).set_pose_solver(KP3D, CAM_K, 50, all_instances=False).prepare()
    assert off.kernel_count() == n0 and off.inst_poses is None
    off.run(frame)
    for a, b in zip(_state(off), want):
        assert a.tobytes() == b.tobytes()
    for _ in range(2):
        on.run(frame)
    replay = _state(on) + [on.inst_poses.cpu().numpy().copy()]
    for a, b in zip(replay[:5], want):
        assert a.tobytes() == b.tobytes()                            # the tail's outputs are untouched
    eager = mk(False).set_pose_solver(KP3D, CAM_K, 50, all_instances=True)
    eager.run(frame)
    got = _state(eager) + [eager.inst_poses.cpu().numpy().copy()]
    for a, b in zip(got, replay):
        assert a.tobytes() == b.tobytes()                            # graph replay = eager run
    inst = replay[5]
    np.testing.assert_array_equal(_bits64(inst[0]), _bits64(replay[2][0]))
    m = int(replay[4][1])
    for j in range(max(m, 1), 3):
        assert inst[j, 0] == 1 and np.isnan(inst[j, 2:14]).all()
    # the stand-alone launch on the pipeline's outputs gives the same rows
    alone = ops.pose_instances(on.merged[None], on.info[None], on.poses, KP3D, CAM_K, 50)[0].cpu().numpy()
    np.testing.assert_array_equal(_bits64(alone), _bits64(inst))
    dev = finish_candidate_pose_record(replay[0], n, replay[2][0], replay[3], replay[4], "f.png", inst_poses=inst)
    host = finish_candidate_records(rows, n, "f.png", KP3D, CAM_K, 50, all_instances=True)
    print("pipeline frame: %d candidates, %d merged poses" % (n, m))
    _hold_to_host_bar(_same_dict(dev, host, "pipeline"))


def test_packed_row_carries_the_instance_rows(nets, tmp_path, cuda):
    from betapose_amd.frame_loader import FrameLoader
    det, pose = nets
    frames = synth.synth_frames(3, 321)
    paths = _write_pngs(tmp_path, frames)
    assert candidate_row_floats(3, True, True) > candidate_row_floats(3, True) == candidate_row_floats(3, True, False)
    runner = StreamedRunner(det, pose, 480, 640, streams=2, pose_solver=(KP3D, CAM_K, 50), candidates=3, nms_conf=NMS_CONF,
                            all_instances=True)
    got = {}
    ld = FrameLoader(paths, threads=2, depth=8)
    assert runner.run(ld, lambda i, row: got.__setitem__(i, row)) == 3
    ld.close()
    cp = CandidatePipeline(det, pose, 480, 640, candidates=3, nms_conf=NMS_CONF).set_pose_solver(KP3D, CAM_K, 50, all_instances=True)
    for i in range(3):
        assert got[i].shape == (candidate_row_floats(3, True, True),)
        cp.run(frames[i])
        res, cnt, prow, mg, info = _state(cp)
        inst = cp.inst_poses.cpu().numpy()
        old = unpack_candidate_row(got[i][:candidate_row_floats(3, True)], 3, True)     # every existing offset is unchanged
        new = unpack_candidate_row(got[i], 3, True, instances=True)
        assert len(old) == 5 and len(new) == 6
        for a, b in zip(old, new[:5]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        assert new[1] == int(cnt[0])
        for a, b in zip((new[0], new[2], new[3], new[4], new[5]), (res, prow[0], mg, info, inst)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()
    with pytest.raises(ValueError):
        StreamedRunner(det, pose, 480, 640, streams=1, candidates=3, all_instances=True)      # no pose solver


# ------------------------------------------------------------------ harness
def _evaluate(outdir, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--synthetic", "4", "--sp", "--outdir", str(outdir)] + list(flags),
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(os.path.join(str(outdir), "Betapose-results.json")).read()


def test_evaluate_all_instances(tmp_path):
    host = json.loads(_evaluate(tmp_path / "host", "--candidates", "3", "--all_instances"))
    dev = json.loads(_evaluate(tmp_path / "dev", "--candidates", "3", "--all_instances", "--device_pnp"))
    assert len(host) == len(dev) > 0
    for x, y in zip(host, dev):
        assert x["image_id"] == y["image_id"] and x["keypoints"] == y["keypoints"] and x["score"] == y["score"]
        assert ("cam_R" in x) == ("cam_R" in y)
        if "cam_R" in x:
            d = max(np.abs(np.subtract(x["cam_R"], y["cam_R"])).max(), np.abs(np.subtract(x["cam_t"], y["cam_t"])).max())
            print("%s: |R, t| difference host / device instances %.3g" % (x["image_id"], d))
            assert d <= RT_TOL
    # without the flag: today's JSON -- every entry of an image carries result[0]'s pose
    plain = _evaluate(tmp_path / "plain", "--candidates", "3")
    pl = json.loads(plain)
    assert len(pl) == len(host)
    first = {}
    for x, h in zip(pl, host):
        first.setdefault(x["image_id"], x)
        assert x["keypoints"] == h["keypoints"] and x["score"] == h["score"]
        assert x.get("cam_R") == first[x["image_id"]].get("cam_R") and x.get("cam_t") == first[x["image_id"]].get("cam_t")
    for x, h in zip(pl, host):
        if first[x["image_id"]] is x:
            assert x.get("cam_R") == h.get("cam_R") and x.get("cam_t") == h.get("cam_t")


def test_evaluate_all_instances_needs_candidates(tmp_path):
    for script in ("evaluate.py", "occlusion_evaluate.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--synthetic", "2", "--outdir", str(tmp_path), "--all_instances"],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode != 0 and "--all_instances" in r.stderr and "--candidates" in r.stderr, r.stderr
