#!/usr/bin/env python3
"""Recorded outputs of the host RANSAC PnP (bp_solve_pnp_ransac) on the inputs of
tests/test_pnp.py::test_ransac_variant_rejects_planted_outliers plus a few other (n, trials, confidence) settings, so
that a change of the solver's internals can be checked for bit-identical results.  Run it with the library of the
commit whose behaviour is to be pinned (BP_LIB selects another build).  Writes tests/golden/pnp_ransac_host.npz."""
import os, sys
import numpy as np
from scipy.spatial.transform import Rotation as Rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from betapose_amd._lib import BetaposeHipError  # noqa: E402
from betapose_amd.ops import solve_pnp_ransac  # noqa: E402
from betapose_amd.synth import CAM_K, synth_kp3d  # noqa: E402


def project(P, R, t):
    uv = (P @ R.T + t) @ CAM_K.T
    return uv[:, :2] / uv[:, 2:]


def poses(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        R = Rot.from_rotvec(rng.normal(0, 0.9, 3)).as_matrix()
        t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 1.5)])
        yield R, t, rng


out = {}
P = synth_kp3d(50) * 3.0
k = 0
for R, t, rng in poses(20, 8):          # the inputs of the existing test, in its order of random draws
    uv = project(P, R, t) + rng.normal(0, 0.5, (50, 2))
    bad = rng.choice(50, 10, replace=False)
    uv[bad] += rng.uniform(30, 120, (10, 2)) * rng.choice([-1, 1], (10, 2))
    R1, t1, inl = solve_pnp_ransac(P, uv, CAM_K, reprojection_error=12.0)
    out["a%d_uv" % k], out["a%d_R" % k], out["a%d_t" % k], out["a%d_inl" % k] = uv, R1, t1, inl
    k += 1
out["a_P"], out["a_count"] = P, np.array(k)
# other point counts, trial limits and confidences (the early stop and the trial limit take other paths)
k = 0
for n, share, trials, conf, err in ((20, 0.4, 100, 0.99, 12.0), (10, 0.2, 100, 0.999, 8.0), (7, 0.0, 100, 0.5, 12.0),
                                    (50, 0.6, 30, 0.99, 12.0), (50, 0.0, 1, 0.99, 12.0), (6, 0.0, 100, 0.99, 12.0),
                                    (30, 0.4, 500, 0.9999, 4.0)):
    for R, t, rng in poses(3, 100 + k):
        Pn = synth_kp3d(50)[:n] * 3.0
        uv = project(Pn, R, t) + rng.normal(0, 0.5, (n, 2))
        nb = int(round(share * n))
        bad = rng.choice(n, nb, replace=False)
        uv[bad] += rng.uniform(30, 120, (nb, 2)) * rng.choice([-1, 1], (nb, 2))
        try:
            R1, t1, inl = solve_pnp_ransac(Pn, uv, CAM_K, reprojection_error=err, iterations=trials, confidence=conf)
        except BetaposeHipError:           # no consensus: recorded as such (NaN pose, empty mask)
            R1, t1, inl = np.full((3, 3), np.nan), np.full((3, 1), np.nan), np.zeros(n, bool)
        out["b%d_P" % k], out["b%d_uv" % k], out["b%d_prm" % k] = Pn, uv, np.array([err, trials, conf])
        out["b%d_R" % k], out["b%d_t" % k], out["b%d_inl" % k] = R1, t1, inl
        k += 1
out["b_count"] = np.array(k)
path = os.path.join(ROOT, "tests", "golden", "pnp_ransac_host.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
