#!/usr/bin/env python3
"""The depth refinement at the size of one Occlusion-LineMod object's evaluation: P = 1 214 poses of a closed synthetic
mesh of 20 000 vertices (bench_vsd.py's sphere, 39 600 triangles, about 100 x 100 px of a 640 x 480 image), each started
a few millimetres and about a degree off the pose its test depth image was rendered from.  bp_refine_depth (8 iterations,
default chunk) and bp_icp_normal_equations (one render and one accumulation) are timed with HIP events (median of 20 after
a warm-up).  bp_icp_normal_equations on a one-triangle mesh isolates the clear and accumulate passes, whose bytes (one f32
z-buffer written and read, the test image read where something was drawn) give the accumulate pass's share of a step.
The host twin is timed on a few poses and scaled to P, and compared with the device on those.  One JSON line; ``--out
FILE`` also writes it there (profiles/).

    python tools/bench_refine.py [--out profiles/refine_bench.json]
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
from bench_vsd import H, P, RADIUS, T, W, sphere_mesh, timed  # noqa: E402

ITERATIONS = 8
HOST_POSES = 2


def main():
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    cam = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    K = np.ascontiguousarray(cam).reshape(9)
    rng = np.random.default_rng(0)
    gt = np.ascontiguousarray(poses(rng, P)[0][:, :3])
    v, f = sphere_mesh()
    v = v * [1.0, 0.8, 0.6]                        # an ellipsoid: a sphere leaves the rotation to the noise
    index = (np.arange(P) % T).astype(np.int32)
    gt[:] = gt[index]                              # pose p belongs to test image p % T
    depth = metrics.render_depth(gt[:T], v, f, cam, (H, W), dev)[0].astype(np.float64)
    test = np.round(depth * 1000.0).astype(np.uint16)
    start = gt.copy()
    for p in range(P):
        w = rng.normal(size=3) * 0.01
        th = np.linalg.norm(w)
        A = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        start[p, :, :3] = (np.eye(3) + np.sin(th) * A + (1 - np.cos(th)) * A @ A) @ gt[p, :, :3]
        start[p, :, 3] += rng.normal(size=3) * 0.002
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    d_start = torch.from_numpy(start.reshape(P, 12)).to(dev)
    d_test = torch.from_numpy(test.view(np.int16)).to(dev)
    d_idx = torch.from_numpy(index).to(dev)
    d_out = torch.empty((P, 12), dtype=torch.float64, device=dev)
    d_stats = torch.empty((P, 6), dtype=torch.float64, device=dev)
    d_acc = torch.empty((P, metrics.ICP_ACC), dtype=torch.float64, device=dev)

    def mesh_calls(vv, ff):
        d_model, d_faces = torch.from_numpy(np.ascontiguousarray(vv)).to(dev), torch.from_numpy(np.ascontiguousarray(ff)).to(dev)

        def refine():
            _lib.check(L.bp_refine_depth(_lib.ptr(d_model), len(vv), _lib.ptr(d_faces), len(ff), _lib.ptr(d_start), P, _lib.ptr(K),
                                         _lib.ptr(d_test), T, H, W, 0.001, _lib.ptr(d_idx), ITERATIONS, 0.02, 0.25, 32, 0.0, 0.01,
                                         0, _lib.ptr(d_out), _lib.ptr(d_stats), stream.cuda_stream))

        def equations():
            _lib.check(L.bp_icp_normal_equations(_lib.ptr(d_model), len(vv), _lib.ptr(d_faces), len(ff), _lib.ptr(d_start), P,
                                                 _lib.ptr(K), _lib.ptr(d_test), T, H, W, 0.001, _lib.ptr(d_idx), 0.02, 0.25, 0.0,
                                                 0.01, 0, _lib.ptr(d_acc), stream.cuda_stream))
        return refine, equations, (d_model, d_faces)

    refine, equations, keep = mesh_calls(v, f)
    refine_ms, refine_min = timed(refine, stream)
    out, stats = d_out.cpu().numpy().reshape(P, 3, 4), d_stats.cpu().numpy()
    eq_ms, eq_min = timed(equations, stream)
    acc = d_acc.cpu().numpy()
    # the clear and accumulate passes alone: one sliver of a triangle, so transform and rasterise cost next to nothing
    _, bare, keep2 = mesh_calls(np.array([[0.0, 0, 0], [1e-4, 0, 0], [0, 1e-4, 0]]), np.array([[0, 1, 2]], np.int32))
    bare_ms, _ = timed(bare, stream)

    h = HOST_POSES
    t = time.perf_counter()
    ref_out, ref_stats = metrics.refine_poses_depth(start[:h], v, f, cam, test, index[:h], iterations=ITERATIONS)
    host_s = (time.perf_counter() - t) * P / h
    status = stats[:, 5].astype(int)
    line = json.dumps({
        "metric": "refine_depth", "P": P, "n": len(v), "faces": len(f), "H": H, "W": W, "T": T, "iterations": ITERATIONS,
        "device": torch.cuda.get_device_name(dev),
        "refine_ms": round(refine_ms, 3), "refine_ms_min": round(refine_min, 3),
        "render_accumulate_ms": round(eq_ms, 3), "render_accumulate_ms_min": round(eq_min, 3),
        "clear_accumulate_ms": round(bare_ms, 3), "clear_accumulate_zbuffer_bytes": float(P) * H * W * 8,
        "mean_pixels": float(acc[:, 27].mean()),
        "status_counts": {name: int((status == k).sum()) for k, name in enumerate(metrics.ICP_STATUS)},
        "mean_rms_first": float(stats[:, 1].mean()), "mean_rms_last": float(stats[:, 3].mean()),
        "mean_add_before_mm": float(np.mean([metrics.add_err(np.vstack([gt[p], [0, 0, 0, 1]]), np.vstack([start[p], [0, 0, 0, 1]]), v)
                                             for p in range(0, P, 50)]) * 1000),
        "mean_add_after_mm": float(np.mean([metrics.add_err(np.vstack([gt[p], [0, 0, 0, 1]]), np.vstack([out[p], [0, 0, 0, 1]]), v)
                                            for p in range(0, P, 50)]) * 1000),
        "host_poses_timed": h, "host_refine_s_scaled": round(host_s, 1), "refine_speedup": round(host_s / (refine_ms * 1e-3), 1),
        "host_status_equal": bool(np.array_equal(stats[:h, [0, 2, 4, 5]], ref_stats[:, [0, 2, 4, 5]])),
        "host_pose_max_abs_diff": float(np.abs(out[:h] - ref_out).max())})
    print(line)
    del keep, keep2
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
