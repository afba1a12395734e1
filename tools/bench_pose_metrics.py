#!/usr/bin/env python3
"""ADD / ADD-S / 2-D errors of one Occlusion-LineMod object's run (P = 1 214 pose pairs) at n = 5 000 and 20 000 model
vertices: one bp_pose_errors call timed with HIP events (median of 20 after a warm-up), against the host numpy path
timed on a few poses and scaled to P.  One JSON line; ``--out FILE`` also writes it there (profiles/).

    python tools/bench_pose_metrics.py [--out profiles/pose_metrics_bench.json]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from betapose_amd import _lib, metrics  # noqa: E402

P = 1214
FP64_DATASHEET = 78.6e12      # MI355X vector fp64, FLOP/s
FLOPS_PER_PAIR = 8            # 3 sub, 1 mul, 2 FMA (2 each) and the min of the ADD-S inner step
HOST_POSES = {5000: 3, 20000: 1}


def poses(rng, P):
    gt = np.tile(np.eye(4), (P, 1, 1))
    est = gt.copy()
    for p in range(P):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        gt[p, :3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        gt[p, :3, 3] = [rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)]
        est[p, :3, :3] = gt[p, :3, :3]
        est[p, :3, 3] = gt[p, :3, 3] + rng.normal(size=3) * 0.01
    return gt, est


def main():
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    cam = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    K = np.ascontiguousarray(cam).reshape(9)
    rng = np.random.default_rng(0)
    gt, est = poses(rng, P)
    d_gt = torch.from_numpy(np.ascontiguousarray(gt[:, :3].reshape(P, 12))).to(dev)
    d_est = torch.from_numpy(np.ascontiguousarray(est[:, :3].reshape(P, 12))).to(dev)
    d_out = torch.empty(P, 3, dtype=torch.float64, device=dev)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    cases = []
    for n in (5000, 20000):
        model = rng.normal(size=(n, 3)) * [0.05, 0.04, 0.03]
        d_model = torch.from_numpy(model).to(dev)

        def call():
            _lib.check(L.bp_pose_errors(_lib.ptr(d_model), n, _lib.ptr(d_gt), _lib.ptr(d_est), P, _lib.ptr(K), 7,
                                        _lib.ptr(d_out), stream.cuda_stream))
        call()
        ms = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        med = float(np.median(ms))
        pairs = float(n) * n * P
        # host numpy on a few poses, scaled to P (and checked against the device on those)
        h = HOST_POSES[n]
        t = time.perf_counter()
        ref = np.stack(metrics.pose_errors(gt[:h], est[:h], model, cam), axis=1)
        host_s = (time.perf_counter() - t) * P / h
        err = float(np.abs(d_out[:h].cpu().numpy()[:, :2] - ref[:, :2]).max())
        cases.append({"n": n, "device_ms": round(med, 3), "device_ms_min": round(min(ms), 3),
                      "pairs_per_s": pairs / (med * 1e-3),
                      "fp64_datasheet_fraction": round(pairs * FLOPS_PER_PAIR / (med * 1e-3) / FP64_DATASHEET, 4),
                      "host_s_scaled": round(host_s, 1), "host_poses_timed": h, "speedup": round(host_s / (med * 1e-3), 1),
                      "max_abs_err_vs_host_m": err})
    line = json.dumps({"metric": "pose_errors", "P": P, "device": torch.cuda.get_device_name(dev), "cases": cases})
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
