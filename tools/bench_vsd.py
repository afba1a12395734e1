#!/usr/bin/env python3
"""The depth rasteriser and VSD at the size of one Occlusion-LineMod object's evaluation: P = 1 214 pose pairs of a closed
synthetic mesh of 20 000 vertices (a 100 x 200 latitude-longitude sphere, 39 600 triangles) that covers about 100 x 100 px
of a 640 x 480 image.  bp_render_depth (P poses) and bp_vsd_errors (P pairs, default chunk) are timed with HIP events
(median of 20 after a warm-up).  bp_vsd_errors on a one-triangle mesh isolates its clear and reduce passes, whose bytes
(two f32 z-buffers written and read, one uint16 test image read, per pair) give the achieved fraction of the HBM
bandwidth.  The host twin (bp_render_depth_host, metrics.pose_errors_vsd on the host) is timed on a few pairs and scaled
to P, and checked against the device on those.  One JSON line; ``--out FILE`` also writes it there (profiles/).

    python tools/bench_vsd.py [--out profiles/vsd_bench.json]
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

P, T, H, W = 1214, 32, 480, 640
NLAT, NLON = 100, 200
RADIUS = 0.075                # metres: about 100 px across at 0.6 .. 1.2 m with the LineMod camera
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12       # bytes / s: datasheet, and what a float4 copy reaches
HOST_PAIRS = 2


def sphere_mesh():
    """NLAT rings of NLON vertices between two poles' worth of rings (the first and last ring are tiny circles about the
    axis, closed by fans inside them): NLAT * NLON vertices, closed."""
    lat = (np.arange(NLAT) + 0.5) / NLAT * np.pi
    lon = np.arange(NLON) / NLON * 2 * np.pi
    v = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.outer(np.sin(lat), np.sin(lon)),
                  np.outer(np.cos(lat), np.ones(NLON))], axis=-1).reshape(-1, 3) * RADIUS
    f = []
    for i in range(NLAT - 1):
        for j in range(NLON):
            a, b = i * NLON + j, i * NLON + (j + 1) % NLON
            f += [(a, a + NLON, b + NLON), (a, b + NLON, b)]
    for ring in (0, (NLAT - 1) * NLON):             # the two caps
        f += [(ring, ring + j, ring + j + 1) for j in range(1, NLON - 1)]
    return v, np.array(f, dtype=np.int32)


def timed(call, stream):
    call()
    ms = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def main():
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    cam = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    K = np.ascontiguousarray(cam).reshape(9)
    rng = np.random.default_rng(0)
    gt, est = poses(rng, P)
    gt, est = np.ascontiguousarray(gt[:, :3]), np.ascontiguousarray(est[:, :3])
    v, f = sphere_mesh()
    index = (np.arange(P) % T).astype(np.int32)
    # test images: the first T ground truths rendered in front of a wall at 2 m, in millimetres
    wall = metrics.render_depth(gt[:T], v, f, cam, (H, W), dev)[0].astype(np.float64)
    test = np.round(np.where(wall > 0, wall, 2.0) * 1000.0).astype(np.uint16)
    taus = np.ascontiguousarray(metrics.BOP_VSD_TAUS, np.float64)
    diameter = 2 * RADIUS
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    d_gt, d_est = torch.from_numpy(gt.reshape(P, 12)).to(dev), torch.from_numpy(est.reshape(P, 12)).to(dev)
    d_test = torch.from_numpy(test.view(np.int16)).to(dev)
    d_idx = torch.from_numpy(index).to(dev)
    d_depth = torch.empty((P, H, W), dtype=torch.float32, device=dev)
    d_skip = torch.empty(P, dtype=torch.int32, device=dev)
    d_err = torch.empty((P, len(taus)), dtype=torch.float64, device=dev)
    d_cnt = torch.empty((P, 4), dtype=torch.int32, device=dev)

    def mesh_calls(vv, ff):
        d_model, d_faces = torch.from_numpy(np.ascontiguousarray(vv)).to(dev), torch.from_numpy(np.ascontiguousarray(ff)).to(dev)

        def render():
            _lib.check(L.bp_render_depth(_lib.ptr(d_model), len(vv), _lib.ptr(d_faces), len(ff), _lib.ptr(d_gt), P, _lib.ptr(K),
                                         H, W, 0.0, 0.01, _lib.ptr(d_depth), _lib.ptr(d_skip), stream.cuda_stream))

        def vsd():
            _lib.check(L.bp_vsd_errors(_lib.ptr(d_model), len(vv), _lib.ptr(d_faces), len(ff), _lib.ptr(d_gt), _lib.ptr(d_est),
                                       P, _lib.ptr(K), _lib.ptr(d_test), T, H, W, 0.001, _lib.ptr(d_idx),
                                       metrics.BOP_VSD_DELTA, _lib.ptr(taus), len(taus), diameter, 0.0, 0.01, 0, _lib.ptr(d_err),
                                       _lib.ptr(d_cnt), stream.cuda_stream))
        return render, vsd, (d_model, d_faces)

    render, vsd, keep = mesh_calls(v, f)
    render_ms, render_min = timed(render, stream)
    covered = float((d_depth[:8] > 0).float().sum(dim=(1, 2)).mean())
    vsd_ms, vsd_min = timed(vsd, stream)
    err, cnt = d_err.cpu().numpy(), d_cnt.cpu().numpy()
    # the clear and reduce passes alone: one sliver of a triangle, so transform and rasterise cost next to nothing
    _, bare_vsd, keep2 = mesh_calls(np.array([[0.0, 0, 0], [1e-4, 0, 0], [0, 1e-4, 0]]), np.array([[0, 1, 2]], np.int32))
    bare_ms, _ = timed(bare_vsd, stream)
    stream_bytes = float(P) * H * W * (2 * 4 + 2 * 4 + 2)

    h = HOST_PAIRS
    t = time.perf_counter()
    ref_depth = metrics.render_depth(gt[:h], v, f, cam, (H, W))[0]
    host_render_s = (time.perf_counter() - t) * P / h
    t = time.perf_counter()
    ref_err, ref_cnt = metrics.pose_errors_vsd(gt[:h], est[:h], v, f, cam, test, index[:h], diameter)
    host_vsd_s = (time.perf_counter() - t) * P / h
    render()
    same_depth = bool(np.array_equal(d_depth[:h].cpu().numpy().view(np.uint32), ref_depth.view(np.uint32)))
    line = json.dumps({
        "metric": "vsd", "P": P, "n": len(v), "faces": len(f), "H": H, "W": W, "T": T,
        "device": torch.cuda.get_device_name(dev), "mean_covered_px": round(covered, 1),
        "render_ms": round(render_ms, 3), "render_ms_min": round(render_min, 3),
        "vsd_ms": round(vsd_ms, 3), "vsd_ms_min": round(vsd_min, 3),
        "clear_reduce_ms": round(bare_ms, 3), "clear_reduce_bytes": stream_bytes,
        "clear_reduce_fraction_of_hbm_spec": round(stream_bytes / (bare_ms * 1e-3) / HBM_SPEC, 4),
        "clear_reduce_fraction_of_hbm_copy": round(stream_bytes / (bare_ms * 1e-3) / HBM_COPY, 4),
        "host_pairs_timed": h, "host_render_s_scaled": round(host_render_s, 1), "host_vsd_s_scaled": round(host_vsd_s, 1),
        "render_speedup": round(host_render_s / (render_ms * 1e-3), 1), "vsd_speedup": round(host_vsd_s / (vsd_ms * 1e-3), 1),
        "render_bit_identical": same_depth, "vsd_err_equal": bool(np.array_equal(err[:h], ref_err)),
        "vsd_counts_equal": bool(np.array_equal(cnt[:h], ref_cnt)), "mean_vsd_err": float(err.mean())})
    print(line)
    del keep, keep2
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
