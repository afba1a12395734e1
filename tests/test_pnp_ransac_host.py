"""Host side of the RANSAC PnP (no GPU): the sampler and the trials-needed table the host and device solvers share,
the host solver's results unchanged by the move onto them, ``finish_record(..., ransac=...)``, the ``--pnp_ransac`` flag
and the new C prototypes.  The yardstick is ``bp_solve_pnp_ransac`` as it stood before the tables were split out: its
outputs are recorded in tests/golden/pnp_ransac_host.npz (tools/make_golden_ransac.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import helpers
from betapose_amd import _lib, ops
from betapose_amd.pipeline import finish_pose_record, finish_record
from betapose_amd.synth import CAM_K, synth_kp3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP3D = synth_kp3d(50) * 2.0
RANSAC = (12.0, 100, 0.99)


def lcg_samples(n, trials):
    """The sampler restated: 64-bit LCG (Knuth's MMIX constants), fixed seed, the top 31 bits modulo n, duplicates
    within a trial rejected, the state carried from trial to trial."""
    mask = (1 << 64) - 1
    state = 0x9E3779B97F4A7C15
    out = np.zeros((trials, 6), np.int32)
    for it in range(trials):
        row = []
        while len(row) < 6:
            state = (state * 6364136223846793005 + 1442695040888963407) & mask
            c = (state >> 33) % n
            if c not in row:
                row.append(c)
        out[it] = row
    return out


@pytest.mark.parametrize("n,trials", [(50, 100), (20, 100), (10, 37), (7, 100), (6, 5), (64, 300), (50, 1)])
def test_sampler_is_the_restated_lcg(n, trials):
    idx = ops.pnp_ransac_samples(n, trials)
    assert idx.shape == (trials, 6) and idx.dtype == np.int32
    np.testing.assert_array_equal(idx, lcg_samples(n, trials))
    assert idx.min() >= 0 and idx.max() < n
    assert all(len(set(r)) == 6 for r in idx.tolist())
    # a shorter table is a prefix of a longer one: the state is carried, nothing depends on the trial count
    np.testing.assert_array_equal(ops.pnp_ransac_samples(n, trials + 3)[:trials], idx)


def test_trials_needed_is_the_update_of_the_reference_loop():
    """RANSACUpdateNumIters restated with Python's libm (the same C library as the host solver's)."""
    import math
    for n, conf in ((50, 0.99), (10, 0.999), (7, 0.5), (64, 0.99)):
        need = ops.pnp_ransac_trials_needed(n, conf)
        assert need.shape == (n + 1,)
        for cnt in range(n + 1):
            ep = 1.0 - cnt / n
            num = math.log(max(1.0 - conf, 2.2250738585072014e-308))
            den = math.log(max(1.0 - math.pow(1.0 - ep, 6), 2.2250738585072014e-308))
            want = math.ceil(num / den) if den < 0 and num / den < 2 ** 31 - 1 else 2 ** 31 - 1
            assert int(need[cnt]) == want, (n, conf, cnt)
        assert need[0] == 2 ** 31 - 1 and need[n] == 1 and np.all(np.diff(need[1:].astype(np.int64)) <= 0)


def test_host_solver_is_bit_identical_to_the_recorded_parent():
    g = helpers.golden("pnp_ransac_host.npz")
    P = g["a_P"]
    assert int(g["a_count"]) == 20
    for k in range(int(g["a_count"])):      # the inputs of test_pnp.py::test_ransac_variant_rejects_planted_outliers
        R, t, inl = ops.solve_pnp_ransac(P, g["a%d_uv" % k], CAM_K, reprojection_error=12.0)
        assert np.array_equal(R, g["a%d_R" % k]) and np.array_equal(t, g["a%d_t" % k]) and np.array_equal(inl, g["a%d_inl" % k]), k
    failed = 0
    for k in range(int(g["b_count"])):      # other point counts, trial limits, confidences; two of them without consensus
        err, trials, conf = g["b%d_prm" % k]
        if np.isnan(g["b%d_R" % k]).any():
            with pytest.raises(_lib.BetaposeHipError):
                ops.solve_pnp_ransac(g["b%d_P" % k], g["b%d_uv" % k], CAM_K, err, int(trials), conf)
            failed += 1
            continue
        R, t, inl = ops.solve_pnp_ransac(g["b%d_P" % k], g["b%d_uv" % k], CAM_K, err, int(trials), conf)
        assert np.array_equal(R, g["b%d_R" % k]) and np.array_equal(t, g["b%d_t" % k]) and np.array_equal(inl, g["b%d_inl" % k]), k
    assert failed == 2


def _record(seed, n_out=12, det=True, low=False):
    """A frame record whose 50 key points are the heat-map cells nearest to the projection of KP3D under a seeded pose
    (crop window 200..420 x 120..400: 3.5 frame pixels per heat-map cell), ``n_out`` of them moved far away."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(316, np.float32)
    rec[0] = np.array([3 if det else -1], np.int32).view(np.float32)[0]
    rec[5] = 0.75
    rec[8:12] = [200.0, 120.0, 420.0, 400.0]
    rec[12:16] = [210.0, 130.0, 410.0, 390.0]
    R = Rot.from_rotvec(rng.normal(0, 0.6, 3)).as_matrix()
    t = np.array([-0.02, 0.025, 0.8]) + rng.normal(0, 0.01, 3)
    uv = (KP3D @ R.T + t) @ CAM_K.T
    uv = uv[:, :2] / uv[:, 2:]
    x = np.rint((uv[:, 0] + 0.3 - 198.0) / 3.5 - 0.2).astype(np.int64)
    y = np.rint((uv[:, 1] + 0.3 - 120.0) / 3.5 - 0.2).astype(np.int64)
    bad = rng.choice(50, n_out, replace=False)
    x[bad] += rng.integers(8, 25, n_out) * rng.choice([-1, 1], n_out)
    y[bad] += rng.integers(8, 25, n_out) * rng.choice([-1, 1], n_out)
    x, y = np.clip(x, 1, 62), np.clip(y, 1, 78)
    kp = rec[16:].reshape(50, 6)
    kp[:, 0] = (y * 64 + x).astype(np.int32).view(np.float32)
    kp[:, 1] = rng.uniform(0.05, 0.29, 50) if low else rng.uniform(0.3, 0.95, 50)
    kp[:, 2:] = 0.1                        # equal neighbours: no quarter-cell offset
    return rec, bad


def _pruned(out, left):
    """The points finish_record's own pruning keeps, from its result dict (dataloader.py:718-722)."""
    sc = np.array(out["result"][0]["kp_score"][:, 0])
    k2 = np.array(out["result"][0]["keypoints"])
    k3 = np.array(KP3D)
    orig = np.arange(50)
    while len(k2) > left:
        d = int(np.argmin(sc))
        sc, k2, k3, orig = np.delete(sc, d), np.delete(k2, d, axis=0), np.delete(k3, d, axis=0), np.delete(orig, d)
    return k3, k2, orig


@pytest.mark.parametrize("left", [50, 10])
def test_finish_record_with_ransac_is_the_host_solver_on_the_pruned_points(left):
    for seed in (1, 2, 3):
        rec, bad = _record(seed)
        plain = finish_record(rec, "a.png", KP3D, CAM_K, left)
        assert set(plain) == {"imgname", "result", "boxes", "scores", "yolo_index", "cam_R", "cam_t"}      # today's dict
        plain2 = finish_record(rec, "a.png", KP3D, CAM_K, left, ransac=None)
        assert plain.keys() == plain2.keys() and np.array_equal(plain["cam_R"], plain2["cam_R"]) and np.array_equal(plain["cam_t"], plain2["cam_t"])
        out = finish_record(rec, "a.png", KP3D, CAM_K, left, ransac=RANSAC)
        assert set(out) == set(plain) | {"pnp_inliers"}
        k3, k2, orig = _pruned(out, left)
        R, t, inl = ops.solve_pnp_ransac(k3, k2, CAM_K, *RANSAC)
        assert np.array_equal(out["cam_R"], R) and np.array_equal(out["cam_t"], t)
        assert out["pnp_inliers"].dtype == bool and np.array_equal(out["pnp_inliers"], inl) and inl.shape == (min(left, 50),)
        # the planted outliers that survived the pruning are rejected, most of the others kept
        assert not inl[np.isin(orig, bad)].any() and inl.sum() >= 0.6 * len(inl)
        for k in ("result", "boxes", "scores"):
            np.testing.assert_equal(out[k], plain[k])
    rec, _ = _record(4, det=False)
    assert finish_record(rec, "b.png", KP3D, CAM_K, left, ransac=RANSAC) == finish_record(rec, "b.png", KP3D, CAM_K, left)
    rec, _ = _record(5, low=True)            # dropped by pPose-NMS: nothing to solve
    out = finish_record(rec, "c.png", KP3D, CAM_K, left, ransac=RANSAC)
    assert out["result"] == [] and out["cam_R"] == [] and "pnp_inliers" not in out


def test_finish_pose_record_decodes_the_inlier_slot():
    rec, _ = _record(1)
    out = finish_record(rec, "a.png", KP3D, CAM_K, 10, ransac=RANSAC)
    row = np.zeros(166)
    row[1] = 10
    row[2:11], row[11:14] = out["cam_R"].reshape(9), out["cam_t"].reshape(3)
    row[14] = out["result"][0]["proposal_score"][0]
    row[16:] = np.concatenate([out["result"][0]["keypoints"], out["result"][0]["kp_score"]], axis=1).astype(np.float64).reshape(150)
    row[15] = float(sum(1 << j for j in range(10) if out["pnp_inliers"][j]))
    got = finish_pose_record(rec, row, "a.png")
    assert got.keys() == out.keys() and np.array_equal(got["pnp_inliers"], out["pnp_inliers"]) and got["pnp_inliers"].dtype == bool
    row[15] = 0.0                             # RANSAC off: today's keys
    assert "pnp_inliers" not in finish_pose_record(rec, row, "a.png")
    row[1], row[15] = 50, float((1 << 50) - 1 - (1 << 49) - 1)      # 50 bits are exact in a double
    m = finish_pose_record(rec, row, "a.png")["pnp_inliers"]
    assert m.shape == (50,) and not m[0] and not m[49] and m[1:49].all()


def test_no_consensus_raises_as_an_unsolvable_pnp_does():
    rec, _ = _record(6, n_out=50)
    with pytest.raises(_lib.BetaposeHipError):
        finish_record(rec, "a.png", KP3D, CAM_K, 50, ransac=(0.5, 100, 0.99))


def test_flag_parses():
    from betapose_amd.opt import build_parser
    p = build_parser()
    assert p.parse_args([]).pnp_ransac is None
    assert p.parse_args(["--pnp_ransac"]).pnp_ransac == 12.0
    assert p.parse_args(["--pnp_ransac", "20"]).pnp_ransac == 20.0
    ns = p.parse_args(["--pnp_ransac", "--device_pnp", "--fused"])
    assert ns.pnp_ransac == 12.0 and ns.device_pnp and ns.fused
    for script in ("evaluate.py", "occlusion_evaluate.py"):
        assert "args.pnp_ransac" in open(os.path.join(ROOT, script)).read(), script



def test_new_prototypes_compile_as_c99(tmp_path):
    header = helpers.header_code()
    for name in ("bp_pnp_ransac_samples", "bp_pnp_ransac_trials_needed", "bp_pnp_ransac_workspace_bytes",
                 "bp_solve_pnp_ransac_batch", "bp_pipeline_set_pose_ransac", "bp_pose_ransac_workspace_bytes",
                 "bp_pose_from_records_ransac"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES
    _lib.lib()
    src = os.path.join(ROOT, "examples", "pnp_ransac_abi_check.c")
    libdir = os.path.join(ROOT, "betapose_amd")
    exe = str(tmp_path / "ransac_abi")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L" + libdir, "-lbetapose_hip", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
