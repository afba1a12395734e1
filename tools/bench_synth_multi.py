#!/usr/bin/env python3
"""What the instance masks of multi-object scenes cost: 64 scenes at 640 x 480 of J = 8 copies of
bench_vsd.py's closed mesh (20 000 vertices, 39 996 triangles; 7.5 cm radius down to half of it), the LineMod camera,
every object at its own sample_poses stream.  Timed alone on device-resident data with HIP events (median of 20 after
3 warm-up calls, with the minimum and the maximum):

  ``instances``   bp_synth_instances on the stack of the 8 x 64 lone renders.  Its bytes are given twice: ``needed``, every
                  input read and every output written once ((4 J + 5) per pixel), and ``touched``, what the two passes
                  request (the winner pass reads the stack and writes ids and depth, the statistics pass reads the stack
                  and, per object, the ids again: (9 J + 5) per pixel); both against the 6.29 TB/s copy rate the other
                  synthesiser kernels are quoted against.
  ``mask_boxes``  the route it replaces, on entry points that were there before: J calls of bp_mask_boxes, object j's
                  lone renders against the scene depth (visibility by depth test with BOP's tolerance, no owner image).

synthesize_multi is timed end to end on the device (64 scenes) and on the host (a few scenes, scaled to 64 and checked
against the device's).  One JSON line; ``--out FILE`` also writes it there (profiles/).

    python tools/bench_synth_multi.py [--out profiles/synth_multi_bench.json]
"""
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from betapose_amd import _lib, metrics, synth  # noqa: E402
from bench_vsd import RADIUS, sphere_mesh  # noqa: E402

I, H, W, J = 64, 480, 640, 8
HOST_SCENES = 2
COPY_FLOOR_TBS = 6.29
SEED = 0
SCALES = [1.0 - 0.5 * j / (J - 1) for j in range(J)]


def timed(call, stream, warmup=3, runs=20):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


def main():
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    cam = np.array(synth.CAM_K, dtype=np.float64)
    K = np.ascontiguousarray(cam).reshape(9)
    rng = np.random.default_rng(0)
    v, f = sphere_mesh()
    meshes = [(v * s, f, rng.integers(0, 256, size=(len(v), 3), dtype=np.uint8)) for s in SCALES]
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_alone = torch.empty((J, I, H, W), dtype=torch.float32, device=dev)
    d_skip = torch.empty(I, dtype=torch.int32, device=dev)
    d_f = up(f)
    for j, (mv, _, _) in enumerate(meshes):
        poses = synth.sample_poses(I, cam, (H, W), RADIUS * SCALES[j], SEED, distance=(0.6, 1.2), stream=j)
        _lib.check(L.bp_render_depth(_lib.ptr(up(mv)), len(mv), _lib.ptr(d_f), len(f), _lib.ptr(up(poses.reshape(I, 12))), I,
                                     _lib.ptr(K), H, W, 0.0, 0.01, _lib.ptr(d_alone[j]), _lib.ptr(d_skip), s))
    d_present = torch.ones((I, J), dtype=torch.uint8, device=dev)
    d_ids = torch.empty((I, H, W), dtype=torch.uint8, device=dev)
    d_depth = torch.empty((I, H, W), dtype=torch.float32, device=dev)
    d_stats = torch.empty((I, J, synth.INSTANCE_STATS), dtype=torch.int32, device=dev)
    d_boxes = torch.empty((J, I, 2, 4), dtype=torch.int32, device=dev)
    d_counts = torch.empty((J, I, 2), dtype=torch.int32, device=dev)
    d_index = torch.arange(I, dtype=torch.int32, device=dev)

    def instances():
        _lib.check(L.bp_synth_instances(_lib.ptr(d_alone), J, I, H, W, _lib.ptr(d_present), _lib.ptr(d_ids), _lib.ptr(d_depth),
                                        _lib.ptr(d_stats), s))

    def mask_boxes():
        for j in range(J):
            _lib.check(L.bp_mask_boxes(_lib.ptr(d_alone[j]), I, H, W, _lib.ptr(K), 0.0, _lib.ptr(d_depth), I, _lib.ptr(d_index),
                                       metrics.BOP_VSD_DELTA, _lib.ptr(d_boxes[j]), _lib.ptr(d_counts[j]), s))

    ms = {"instances": timed(instances, stream), "mask_boxes": timed(mask_boxes, stream)}
    stats = d_stats.cpu().numpy()
    h = HOST_SCENES
    alone_h = np.ascontiguousarray(d_alone[:, :h].cpu().numpy())
    t = time.perf_counter()
    want = synth.instance_masks(alone_h)
    host_instances_s = (time.perf_counter() - t) * I / h
    same = {"instances": bool(np.array_equal(want[0], d_ids[:h].cpu().numpy()) and np.array_equal(want[2], stats[:h]) and
                              want[1].tobytes() == d_depth[:h].cpu().numpy().tobytes())}
    # the two routes count the same covered pixels; they differ in who counts as visible
    same["px_all_equals_mask_boxes"] = bool(np.array_equal(stats[..., 0], d_counts[..., 0].cpu().numpy().T))
    del d_alone, d_depth, d_ids
    torch.cuda.empty_cache()

    run = lambda n, device: synth.synthesize_multi(meshes, cam, (H, W), n, SEED, distance=(0.6, 1.2), device=device)
    run(1, dev)
    t = time.perf_counter()
    scenes = run(I, dev)
    device_s = time.perf_counter() - t
    t = time.perf_counter()
    host = run(h, None)
    host_s = (time.perf_counter() - t) * I / h
    same["synthesize_multi"] = all(np.array_equal(host[k], scenes[k][:h]) for k in host if k != "obj_ids")

    px = I * H * W
    needed, touched = px * (4 * J + 5), px * (9 * J + 5)
    rate = lambda b: round(b / (ms["instances"]["median"] * 1e-3) / 1e12, 3)
    line = json.dumps({
        "metric": "synth_multi", "date": datetime.date.today().isoformat(), "scenes": I, "H": H, "W": W, "objects": J, "n": len(v),
        "faces": len(f), "device": torch.cuda.get_device_name(dev), "ms": ms,
        "instances_bytes": {"needed": needed, "touched": touched},
        "instances_tb_per_s": {"needed": rate(needed), "touched": rate(touched)},
        "instances_fraction_of_copy_floor": {"needed": round(rate(needed) / COPY_FLOOR_TBS, 3), "touched": round(rate(touched) / COPY_FLOOR_TBS, 3)},
        "mask_boxes_over_instances": round(ms["mask_boxes"]["median"] / ms["instances"]["median"], 2),
        "kept": int(scenes["present"].sum()), "dropped": int((~scenes["present"]).sum()),
        "mean_visib_fract_kept": round(float(scenes["visib_fract"][scenes["present"]].mean()), 3),
        "host_scenes_timed": h, "host_instances_s_scaled": round(host_instances_s, 3),
        "synthesize_multi_device_s": round(device_s, 3), "synthesize_multi_host_s_scaled": round(host_s, 3),
        "host_equals_device": same})
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
