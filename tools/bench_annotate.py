#!/usr/bin/env python3
"""Cost of the key-point annotator at LineMod's size: 1 214 poses of a 20 000-vertex mesh with 50 key points at 640 x 480
(one sequence), and 256 x 50 heat-map targets at 80 x 64 (one training batch of the reference's size and a bit).

    python tools/bench_annotate.py [--poses 1214] [--vertices 20000] [--repeat 5] [--no-gpu]

Prints one JSON line.  The host twins are timed with a host clock; the device entry points are timed with device events
around calls on tensors that are already on the device (no copies inside the window), after a warm-up call of the same
shape, best and median of --repeat.  The renders (bp_render_depth) are timed apart from the new kernels, which only read
them.  Bytes are what each kernel has to move, computed from the shapes, so the rates are lower bounds on what the memory
system delivered; they are call rates (launches included), not kernel rates.  Without a GPU the device part is "not
measured"."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from betapose_amd import _lib, annotate as A, metrics, synth  # noqa: E402

H, W = 480, 640


def sphere_mesh(n_target):
    """A UV sphere of about n_target vertices, 5 cm radius."""
    rings = max(4, int(np.sqrt(n_target / 2.0)))
    segs = max(4, int(round(n_target / rings)))
    th = np.pi * (np.arange(rings) + 0.5) / rings
    ph = 2 * np.pi * np.arange(segs) / segs
    v = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(segs))],
                 axis=-1).reshape(-1, 3) * 0.05
    f = []
    for i in range(rings - 1):
        for j in range(segs):
            a, b = i * segs + j, i * segs + (j + 1) % segs
            f += [(a, b, b + segs), (a, b + segs, a + segs)]
    return np.ascontiguousarray(v), np.array(f, dtype=np.int32)


def scene(P, n, seed=5):
    rng = np.random.default_rng(seed)
    v, f = sphere_mesh(n)
    poses = np.tile(np.eye(4)[:3], (P, 1, 1))
    for p in range(P):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        poses[p, :, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                           [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                           [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        d = rng.uniform(0.6, 1.1)
        poses[p, :, 3] = [rng.uniform(-0.2, 0.2) * d, rng.uniform(-0.15, 0.15) * d, d]
    kp = v[rng.choice(len(v), 50, replace=False)]
    return v, f, poses, kp


def host_time(fn, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3)}


def device_time(fn, repeat):
    import torch
    fn()                                           # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3)}


def with_rate(t, nbytes):
    t = dict(t)
    t["MB"] = round(nbytes / 1e6, 2)
    t["GBps_at_best"] = round(nbytes / 1e9 / (t["best_ms"] / 1e3), 1)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=1214)
    ap.add_argument("--vertices", type=int, default=20000)
    ap.add_argument("--chunk", type=int, default=54, help="poses rendered per call (54 x 480 x 640 floats = 2^24 x 4 B)")
    ap.add_argument("--targets", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-gpu", action="store_true")
    args = ap.parse_args()
    v, f, poses, kp = scene(args.poses, args.vertices)
    K = synth.CAM_K
    C = min(args.chunk, args.poses)
    chunk = poses[:C]
    n_chunks = -(-args.poses // C)
    rng = np.random.default_rng(9)
    B, Kp = args.targets, 50
    ul = np.floor(rng.uniform(0, 200, (B, 2))).astype(np.float32)
    br = ul + np.floor(rng.uniform(100, 280, (B, 2))).astype(np.float32)
    parts = rng.uniform(ul[:, None, :] - 10, br[:, None, :] + 10, (B, Kp, 2))
    # bytes each call has to move: the renders are read once by mask_boxes; the key points touch one pixel each
    b_mask = C * H * W * 4 * 2                                           # render + scene depth
    b_kp = C * Kp * (2 * 8 + 8 + 1 + 2 * 4)
    b_vert = len(v) * 3 * 8 + C * (12 * 8 + 4 * 4)                       # the vertices stay in cache across poses
    b_targets = B * Kp * 80 * 64 * 4
    out = {"poses": args.poses, "vertices": len(v), "faces": len(f), "key_points": Kp, "size": [H, W], "chunk": C,
           "chunks_per_sequence": n_chunks, "targets": [B, Kp, 80, 64], "repeat": args.repeat}

    depth = metrics.render_depth(chunk, v, f, K, (H, W))[0]
    scene_d = np.where(depth > 0, depth + np.float32(0.005), np.float32(1.5)).astype(np.float32)
    scene_d[:, :, :200] = 0.4
    host = {"render_chunk": host_time(lambda: metrics.render_depth(chunk, v, f, K, (H, W)), max(1, args.repeat // 2)),
            "keypoints_chunk": host_time(lambda: A.project_keypoints(chunk, kp, K, (H, W), depth, scene_d), args.repeat),
            "mask_boxes_chunk": host_time(lambda: A.mask_boxes(depth, K, scene_d), args.repeat),
            "vertex_boxes_chunk": host_time(lambda: A.vertex_boxes(chunk, v, K, (H, W)), args.repeat),
            "targets": host_time(lambda: A.kpd_targets(parts, ul, br), args.repeat)}
    host["sequence_ms_without_renders"] = round(n_chunks * sum(host[k]["best_ms"] for k in
                                                               ("keypoints_chunk", "mask_boxes_chunk", "vertex_boxes_chunk")), 1)
    host["sequence_ms_renders"] = round(n_chunks * host["render_chunk"]["best_ms"], 1)
    out["host"] = host

    import torch
    if args.no_gpu or not torch.cuda.is_available():
        out["device"] = "not measured"
        print(json.dumps(out))
        return
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Kf = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    d_v, d_f, d_p, d_kp = up(v), up(f), up(chunk.reshape(C, 12)), up(kp)
    d_depth = torch.empty((C, H, W), dtype=torch.float32, device=dev)
    d_skip = torch.empty(C, dtype=torch.int32, device=dev)
    d_scene, d_idx = up(scene_d), up(np.arange(C, dtype=np.int32))
    d_xy = torch.empty((C, Kp, 2), dtype=torch.float64, device=dev)
    d_z = torch.empty((C, Kp), dtype=torch.float64, device=dev)
    d_fl = torch.empty((C, Kp), dtype=torch.uint8, device=dev)
    d_boxes = torch.empty((C, 2, 4), dtype=torch.int32, device=dev)
    d_counts = torch.empty((C, 2), dtype=torch.int32, device=dev)
    d_vb = torch.empty((C, 4), dtype=torch.int32, device=dev)
    d_parts, d_ul, d_br, d_g = up(parts), up(ul), up(br), up(A.gaussian_table(1))
    d_out = torch.empty((B, Kp, 80, 64), dtype=torch.float32, device=dev)
    d_cen = torch.empty((B, Kp, 2), dtype=torch.int32, device=dev)
    ptr, chk = _lib.ptr, _lib.check

    def render():
        chk(lib.bp_render_depth(ptr(d_v), len(v), ptr(d_f), len(f), ptr(d_p), C, ptr(Kf), H, W, 0.0, 0.01, ptr(d_depth),
                                ptr(d_skip), s))

    def keypoints():
        chk(lib.bp_annotate_keypoints(ptr(d_p), C, ptr(d_kp), Kp, ptr(Kf), H, W, 0.0, 0.01, ptr(d_depth), ptr(d_scene), C,
                                      ptr(d_idx), 0.015, 0.015, ptr(d_xy), ptr(d_z), ptr(d_fl), s))

    def boxes():
        chk(lib.bp_mask_boxes(ptr(d_depth), C, H, W, ptr(Kf), 0.0, ptr(d_scene), C, ptr(d_idx), 0.015, ptr(d_boxes),
                              ptr(d_counts), s))

    def vboxes():
        chk(lib.bp_vertex_boxes(ptr(d_p), C, ptr(d_v), len(v), ptr(Kf), H, W, ptr(d_vb), s))

    def targets():
        chk(lib.bp_kpd_targets(ptr(d_parts), ptr(d_ul), ptr(d_br), B, Kp, 320, 256, 80, 64, ptr(d_g), 7, ptr(d_out), ptr(d_cen),
                               None, s))

    render()
    torch.cuda.synchronize()
    assert np.array_equal(d_depth.cpu().numpy().view(np.uint32), depth.view(np.uint32)), "device render differs from the host's"
    d = {"name": torch.cuda.get_device_name(0),
         "render_chunk": device_time(render, args.repeat),
         "keypoints_chunk": with_rate(device_time(keypoints, args.repeat), b_kp),
         "mask_boxes_chunk": with_rate(device_time(boxes, args.repeat), b_mask),
         "vertex_boxes_chunk": with_rate(device_time(vboxes, args.repeat), b_vert),
         "targets": with_rate(device_time(targets, args.repeat), b_targets)}
    d["sequence_ms_without_renders"] = round(n_chunks * sum(d[k]["best_ms"] for k in
                                                            ("keypoints_chunk", "mask_boxes_chunk", "vertex_boxes_chunk")), 1)
    d["sequence_ms_renders"] = round(n_chunks * d["render_chunk"]["best_ms"], 1)
    # and the results the timed calls left behind equal the host's
    torch.cuda.synchronize()
    want = A.project_keypoints(chunk, kp, K, (H, W), depth, scene_d)
    same = np.array_equal(d_xy.cpu().numpy().view(np.uint64), want[0].view(np.uint64)) and \
        np.array_equal(d_fl.cpu().numpy(), want[2]) and \
        np.array_equal(d_boxes.cpu().numpy(), A.mask_boxes(depth, K, scene_d)[0]) and \
        np.array_equal(d_vb.cpu().numpy(), A.vertex_boxes(chunk, v, K, (H, W))) and \
        np.array_equal(d_out.cpu().numpy().view(np.uint32), A.kpd_targets(parts, ul, br)[0].view(np.uint32))
    d["equal_to_host"] = bool(same)
    out["device"] = d
    print(json.dumps(out))


if __name__ == "__main__":
    main()
