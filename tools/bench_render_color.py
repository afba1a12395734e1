#!/usr/bin/env python3
"""The colour renderer next to the depth rasteriser on the same inputs: P = 64 poses of bench_vsd.py's closed synthetic
mesh (20 000 vertices, 39 996 triangles, about 100 x 100 px of a 640 x 480 image), one pose per image.  bp_render_color
and bp_render_depth are timed with HIP events (median of 20 after a warm-up).  ``one_triangle_call_ms`` is a whole
bp_render_color call on a one-triangle mesh: an UPPER BOUND of the clear and resolve passes, since it also holds the call's
arena allocation, its memset, the (empty) transform and visibility launches and the stream synchronise; the kernels' own
times come from a kernel trace of this script (DESIGN.md 3.5 quotes one).  bp_overlay is one kernel and is timed alone.  The host twin is timed on a few poses and scaled to P,
and checked against the device on those.  One JSON line; ``--out FILE`` also writes it there (profiles/).

    python tools/bench_render_color.py [--out profiles/render_color_bench.json]
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
from bench_vsd import sphere_mesh, timed  # noqa: E402

P, H, W = 64, 480, 640
HOST_POSES = 2


def main():
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    cam = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    K = np.ascontiguousarray(cam).reshape(9)
    rng = np.random.default_rng(0)
    gt = np.ascontiguousarray(poses(rng, P)[0][:, :3])
    v, f = sphere_mesh()
    colors = rng.integers(0, 256, size=(len(v), 3), dtype=np.uint8)
    light = np.zeros(3)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    d_poses = torch.from_numpy(gt.reshape(P, 12)).to(dev)
    d_color = torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)
    d_depth = torch.empty((P, H, W), dtype=torch.float32, device=dev)
    d_depth2 = torch.empty((P, H, W), dtype=torch.float32, device=dev)
    d_skip = torch.empty(P, dtype=torch.int32, device=dev)
    d_frames = torch.randint(0, 256, (P, H, W, 3), dtype=torch.uint8, device=dev)
    d_out = torch.empty_like(d_frames)

    def mesh_calls(vv, ff, cc):
        d_model, d_faces = torch.from_numpy(np.ascontiguousarray(vv)).to(dev), torch.from_numpy(np.ascontiguousarray(ff)).to(dev)
        d_cols = torch.from_numpy(np.ascontiguousarray(cc)).to(dev)

        def color():
            _lib.check(L.bp_render_color(_lib.ptr(d_model), len(vv), _lib.ptr(d_faces), len(ff), _lib.ptr(d_cols),
                                         _lib.ptr(d_poses), P, None, P, _lib.ptr(K), H, W, 0.0, 0.01, 0.5, _lib.ptr(light), 0,
                                         _lib.ptr(d_color), _lib.ptr(d_depth), _lib.ptr(d_skip), stream.cuda_stream))

        def depth():
            _lib.check(L.bp_render_depth(_lib.ptr(d_model), len(vv), _lib.ptr(d_faces), len(ff), _lib.ptr(d_poses), P,
                                         _lib.ptr(K), H, W, 0.0, 0.01, _lib.ptr(d_depth2), _lib.ptr(d_skip), stream.cuda_stream))
        return color, depth, (d_model, d_faces, d_cols)

    def overlay():
        _lib.check(L.bp_overlay(_lib.ptr(d_frames), _lib.ptr(d_color), _lib.ptr(d_depth), P, H, W, 128, _lib.ptr(d_out),
                                stream.cuda_stream))

    color, depth, keep = mesh_calls(v, f, colors)
    depth_ms, depth_min = timed(depth, stream)
    color_ms, color_min = timed(color, stream)
    same_depth = bool(torch.equal(d_depth.view(torch.int32), d_depth2.view(torch.int32)))
    covered = float((d_depth[:8] > 0).float().sum(dim=(1, 2)).mean())
    overlay_ms, _ = timed(overlay, stream)
    got_color, got_depth = d_color[:HOST_POSES].cpu().numpy(), d_depth[:HOST_POSES].cpu().numpy()
    # one sliver of a triangle: transform and visibility cost next to nothing, the call's fixed overhead stays
    bare, _, keep2 = mesh_calls(np.array([[0.0, 0, 0], [1e-4, 0, 0], [0, 1e-4, 0]]), np.array([[0, 1, 2]], np.int32),
                                np.zeros((3, 3), np.uint8))
    bare_ms, _ = timed(bare, stream)

    h = HOST_POSES
    t = time.perf_counter()
    ref = metrics.render_color(gt[:h], v, f, colors, cam, (H, W))
    host_s = (time.perf_counter() - t) * P / h
    line = json.dumps({
        "metric": "render_color", "P": P, "n": len(v), "faces": len(f), "H": H, "W": W,
        "device": torch.cuda.get_device_name(dev), "mean_covered_px": round(covered, 1),
        "render_color_ms": round(color_ms, 3), "render_color_ms_min": round(color_min, 3),
        "render_depth_ms": round(depth_ms, 3), "render_depth_ms_min": round(depth_min, 3),
        "color_to_depth_ratio": round(color_ms / depth_ms, 3),
        "one_triangle_call_ms": round(bare_ms, 3), "overlay_ms": round(overlay_ms, 3),
        "host_poses_timed": h, "host_render_color_s_scaled": round(host_s, 4),
        "speedup": round(host_s / (color_ms * 1e-3), 1), "depth_equals_render_depth": same_depth,
        "color_byte_identical": bool(np.array_equal(got_color, ref[0])),
        "depth_bit_identical": bool(np.array_equal(got_depth.view(np.uint32), ref[1].view(np.uint32)))})
    print(line)
    del keep, keep2
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
