#!/usr/bin/env python3
"""MSSD / MSPD of one Occlusion-LineMod object's run (P = 1 214 pose pairs, n = 20 000 model vertices) over symmetry
sets of S = 1, 2, 316 and 632 transforms (none, one discrete, one continuous axis at the BOP step, both): one
bp_pose_errors_sym call timed with HIP events (median of 20 after a warm-up), against the host numpy path timed on a
few poses and scaled to P.  Each case is timed for both errors and for MSSD alone; the fraction of the f64 vector peak
counts 12 FMA-equivalents per (pose, symmetry, vertex) of the MSSD-alone call.  One JSON line; ``--out FILE`` also
writes it there (profiles/).

    python tools/bench_pose_metrics_sym.py [--out profiles/pose_metrics_sym_bench.json]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from betapose_amd import _lib, metrics  # noqa: E402
from bench_pose_metrics import poses  # noqa: E402

P, N = 1214, 20000
FP64_DATASHEET = 78.6e12      # MI355X vector fp64, FLOP/s
FMA_PER_POINT = 12            # 9 for D [x; 1], 3 for the squared length
HOST_POSES = {1: 8, 2: 4, 316: 1, 632: 1}
HALF_TURN_Z = [-1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]
Z_AXIS = [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]


def symmetry_set(S):
    """S = 1: the identity; 2: a half turn; 316 / 632: the 315 steps of a continuous axis (x the half turn) and one
    more element, so the counts are those of the round figures people quote."""
    entry = {}
    if S in (2, 632):
        entry["symmetries_discrete"] = [HALF_TURN_Z]
    if S >= 316:
        entry["symmetries_continuous"] = Z_AXIS
    sym = metrics.symmetry_transforms(entry)
    extra = S - len(sym)
    if extra:       # 316 = 315 + 1, 632 = 630 + 2: pad with quarter turns about x
        q = np.array([[1.0, 0, 0, 0], [0, 0, -1.0, 0], [0, 1.0, 0, 0]])
        sym = np.concatenate([sym, np.stack([q, q * [[1], [-1], [-1]]])[:extra]])
    assert len(sym) == S
    return sym


def main():
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    cam = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    K = np.ascontiguousarray(cam).reshape(9)
    rng = np.random.default_rng(0)
    gt, est = poses(rng, P)
    model = rng.normal(size=(N, 3)) * [0.05, 0.04, 0.03]
    d_model = torch.from_numpy(model).to(dev)
    d_gt = torch.from_numpy(np.ascontiguousarray(gt[:, :3].reshape(P, 12))).to(dev)
    d_est = torch.from_numpy(np.ascontiguousarray(est[:, :3].reshape(P, 12))).to(dev)
    d_out = torch.empty(P, 2, dtype=torch.float64, device=dev)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    cases = []
    for S in (1, 2, 316, 632):
        sym = symmetry_set(S)
        d_sym = torch.from_numpy(np.ascontiguousarray(sym.reshape(S, 12))).to(dev)

        def call(want):
            _lib.check(L.bp_pose_errors_sym(_lib.ptr(d_model), N, _lib.ptr(d_gt), _lib.ptr(d_est), P, _lib.ptr(d_sym), S,
                                            _lib.ptr(K), want, _lib.ptr(d_out), stream.cuda_stream))

        def timed(want):
            call(want)
            ms = []
            for _ in range(20):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call(want)
                b.record(stream)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return float(np.median(ms)), float(min(ms))
        mssd_ms, _ = timed(1)
        med, lo = timed(3)          # leaves both columns in d_out
        points = float(P) * S * N
        # host numpy on a few poses, scaled to P (and checked against the device on those)
        h = HOST_POSES[S]
        t = time.perf_counter()
        ref = np.stack(metrics.pose_errors_sym(gt[:h], est[:h], model, cam, sym), axis=1)
        host_s = (time.perf_counter() - t) * P / h
        got = d_out[:h].cpu().numpy()
        cases.append({"S": S, "device_ms": round(med, 3), "device_ms_min": round(lo, 3), "mssd_only_ms": round(mssd_ms, 3),
                      "points_per_s": points / (med * 1e-3),
                      "mssd_fp64_datasheet_fraction": round(points * FMA_PER_POINT * 2 / (mssd_ms * 1e-3) / FP64_DATASHEET, 4),
                      "host_s_scaled": round(host_s, 1), "host_poses_timed": h, "speedup": round(host_s / (med * 1e-3), 1),
                      "max_abs_err_mssd_m": float(np.abs(got[:, 0] - ref[:, 0]).max()),
                      "max_abs_err_mspd_px": float(np.abs(got[:, 1] - ref[:, 1]).max())})
    by = {c["S"]: c for c in cases}
    line = json.dumps({"metric": "pose_errors_sym", "P": P, "n": N, "device": torch.cuda.get_device_name(dev),
                       "cases": cases, "ms_S316_over_S1": round(by[316]["device_ms"] / by[1]["device_ms"], 2)})
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
