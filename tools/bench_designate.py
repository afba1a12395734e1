#!/usr/bin/env python3
"""Cost of the key-point designator at LineMod's size: a 20 000-vertex mesh (a 50 mm sphere with bumps, in millimetres).

    python tools/bench_designate.py [--vertices 20000] [--repeat 7] [--no-gpu] [--out profiles/designate_bench.json]

Four figures, host twin against device: one octave of 8 scales over all the vertices (sigma0 = 1 mm, about the vertex
spacing), the whole sift_keypoints at the reference's defaults (a Python loop over ten octaves, the voxel grid on the
host, uploads and downloads included on the device side), farthest_points at K = 50, and thin_points from 2 000 points
to 50.  The host twins are timed with a host clock (the two long ones once); the device entry points with device events
around calls on tensors that are already on the device, after a warm-up call of the same shape, best and median of
--repeat.  The results the timed device calls left behind are compared with the host's.  Prints one JSON line and
writes it to --out.  Without a GPU the device part is "not measured"."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from betapose_amd import _lib, designate as D  # noqa: E402


def bumpy_sphere(n_target, seed=4):
    """About n_target vertices of a UV sphere of 50 mm radius with a dozen Gaussian bumps of a few millimetres."""
    rings = max(4, int(np.sqrt(n_target / 2.0)))
    segs = max(4, int(round(n_target / rings)))
    th = np.pi * (np.arange(rings) + 0.5) / rings
    ph = 2 * np.pi * np.arange(segs) / segs
    u = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(segs))],
                 axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    r = np.full(len(u), 50.0)
    for _ in range(12):
        c = rng.normal(size=3)
        c /= np.linalg.norm(c)
        r += rng.uniform(-4.0, 4.0) * np.exp(-(np.arccos(np.clip(u @ c, -1, 1)) * 50.0) ** 2 / (2 * rng.uniform(3.0, 8.0) ** 2))
    return np.ascontiguousarray(u * r[:, None])


def host_time(fn, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3), "repeat": repeat}


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
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3), "repeat": repeat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=20000)
    ap.add_argument("--thin_from", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "designate_bench.json"))
    args = ap.parse_args()
    v = bumpy_sphere(args.vertices)
    n, ns, K, keep = len(v), 8, 50, 50
    scales = D.octave_scales(1.0, 0, ns - 3)
    thin_in = np.ascontiguousarray(v[np.random.default_rng(8).choice(n, args.thin_from, replace=False)])
    out = {"vertices": n, "octave": {"ns": ns, "sigma0": 1.0, "k": 25, "min_contrast": 0.005}, "fps_K": K, "thin": [len(thin_in), keep],
           "repeat": args.repeat}

    res = {}
    host = {"octave": host_time(lambda: res.__setitem__("octave", D.sift_octave(v, 2, scales, 25, 0.005)), 1),
            "sift_keypoints_defaults": host_time(lambda: res.__setitem__("sift", D.sift_keypoints(v, return_sizes=True)), 1),
            "farthest_points": host_time(lambda: res.__setitem__("fps", D.farthest_points(v, K)), args.repeat),
            "thin_points": host_time(lambda: res.__setitem__("thin", D.thin_points(thin_in, keep)), args.repeat)}
    out["host"] = host
    out["octave_sizes_defaults"] = res["sift"][1]
    out["keypoints_defaults"] = int(len(res["sift"][0]))
    out["octave_flags"] = int((res["octave"][1] != 0).sum())

    import torch
    if args.no_gpu or not torch.cuda.is_available():
        out["device"] = "not measured"
    else:
        lib, ptr, chk = _lib.lib(), _lib.ptr, _lib.check
        dev = torch.device("cuda:0")
        s = torch.cuda.current_stream().cuda_stream
        d_v, d_thin = torch.from_numpy(v).to(dev), torch.from_numpy(thin_in).to(dev)
        d_dog = torch.empty((n, ns - 1), dtype=torch.float64, device=dev)
        d_fl = torch.empty((n, ns - 3), dtype=torch.int8, device=dev)
        d_idx = torch.empty(K, dtype=torch.int32, device=dev)
        d_d2 = torch.empty(K, dtype=torch.float64, device=dev)
        d_alive = torch.empty(len(thin_in), dtype=torch.uint8, device=dev)
        d_state = torch.empty(2, dtype=torch.int32, device=dev)
        dres = {}
        d = {"name": torch.cuda.get_device_name(0),
             "octave": device_time(lambda: chk(lib.bp_sift_octave(ptr(d_v), n, 2, ptr(scales), ns, 25, 0.005, ptr(d_dog),
                                                                  ptr(d_fl), s)), args.repeat),
             "sift_keypoints_defaults": device_time(
                 lambda: dres.__setitem__("sift", D.sift_keypoints(v, return_sizes=True, device=dev)), 3),
             "farthest_points": device_time(lambda: chk(lib.bp_farthest_points(ptr(d_v), n, K, -1, ptr(d_idx), ptr(d_d2), s)),
                                            args.repeat),
             "thin_points": device_time(lambda: chk(lib.bp_thin_points(ptr(d_thin), len(thin_in), keep, ptr(d_alive),
                                                                       ptr(d_state), s)), args.repeat)}
        torch.cuda.synchronize()
        same = np.array_equal(d_dog.cpu().numpy().view(np.uint64), res["octave"][0].view(np.uint64)) and \
            np.array_equal(d_fl.cpu().numpy(), res["octave"][1]) and \
            np.array_equal(dres["sift"][0].view(np.uint64), res["sift"][0].view(np.uint64)) and \
            np.array_equal(d_idx.cpu().numpy(), res["fps"][0]) and \
            np.array_equal(d_d2.cpu().numpy().view(np.uint64), res["fps"][1].view(np.uint64)) and \
            np.array_equal(np.flatnonzero(d_alive.cpu().numpy()), res["thin"]) and \
            int(d_state.cpu().numpy()[0]) == len(thin_in) - keep
        d["equal_to_host"] = bool(same)
        for k in ("octave", "sift_keypoints_defaults", "farthest_points", "thin_points"):
            d[k]["host_over_device"] = round(host[k]["best_ms"] / d[k]["best_ms"], 2)
        out["device"] = d
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
