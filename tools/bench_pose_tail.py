#!/usr/bin/env python3
"""Cost of the device pose tail (csrc/pose_tail.hip) on one GPU.  One JSON line; ``--out FILE`` also
writes it there (profiles/pose_tail_bench.json):

  * tail kernel per launch at batch 1 and 28 (bp_pose_from_records on real pipeline records): HIP events around each
    launch, median of 20 after a warm-up;
  * host finish_record against finish_pose_record, microseconds per frame;
  * lone-frame latency (FramePipeline.run, batch 1) with and without the tail;
  * StreamedRunner frames/s over written PNGs, host tail against device tail, at (bf16x3, 4 streams, batch 1) and
    (f16, 3 streams, batch 28).

``--kernel-only`` launches the tail 20 times at batch 1 and 28 and prints nothing else: the run to put under
``rocprofv3 --kernel-trace --stats`` as the cross-check of the event timing.

    python tools/bench_pose_tail.py [--out profiles/pose_tail_bench.json] [--kernel-only]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import helpers  # noqa: E402
from betapose_amd import ops, synth  # noqa: E402
from betapose_amd.darknet import Darknet  # noqa: E402
from betapose_amd.kpd import FastPoseHIP  # noqa: E402
from betapose_amd.pipeline import FramePipeline, StreamedRunner, finish_pose_record, finish_record  # noqa: E402

KP3D, K, LEFT = synth.synth_kp3d(50), synth.CAM_K, 50


def engines(max_batch, mode):
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416, max_batch=max_batch).load_stream(helpers.yolo_stream()).cuda()
    pose = FastPoseHIP(helpers.kpd_state_dict(), n_classes=50, max_batch=max_batch).cuda()
    det.set_precision(mode)
    pose.set_precision(mode)
    return det, pose


def records(n):
    det, pose = engines(1, "bf16x3")
    pipe = FramePipeline(det, pose, 480, 640, batch=1)
    return np.stack([pipe.run(f)[0] for f in synth.synth_frames(n, 4321)])


def tail_ms(recs, B, reps=20):
    r = torch.from_numpy(np.resize(recs, (B, recs.shape[1]))).cuda()
    for _ in range(3):
        ops.pose_from_records(r, KP3D, K, LEFT)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.pose_from_records(r, KP3D, K, LEFT)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    rows = ops.pose_from_records(r, KP3D, K, LEFT).cpu().numpy()
    return float(np.median(ts)), rows


def host_us(recs, rows):
    t = time.perf_counter()
    for i, rec in enumerate(recs):
        finish_record(rec, "%d.png" % i, KP3D, K, LEFT)
    th = (time.perf_counter() - t) / len(recs)
    t = time.perf_counter()
    for i, rec in enumerate(recs):
        finish_pose_record(rec, rows[i], "%d.png" % i)
    td = (time.perf_counter() - t) / len(recs)
    return th * 1e6, td * 1e6


def lone_frame_ms(reps=20):
    det, pose = engines(1, "bf16x3")
    pipe = FramePipeline(det, pose, 480, 640, batch=1)
    frame = synth.synth_frames(1, 99)[0]
    out = {}
    for name, on in (("without_tail", False), ("with_device_tail", True)):
        if on:
            pipe.set_pose_solver(KP3D, K, LEFT)
        else:
            pipe.set_pose_solver(None)
        for _ in range(3):
            pipe.run(frame)
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            pipe.run(frame)
            if on:
                pipe.poses.cpu()
            ts.append((time.perf_counter() - t) * 1e3)
        out[name] = float(np.median(ts))
    return out


def streamed_fps(paths, mode, streams, batch):
    from betapose_amd.frame_loader import FrameLoader
    det, pose = engines(batch, mode)
    out = {}
    for name in ("host_tail", "device_tail"):
        dev = name == "device_tail"
        runner = StreamedRunner(det, pose, 480, 640, streams=streams, batch=batch,
                                pose_solver=(KP3D, K, LEFT) if dev else None)
        names = [os.path.basename(p) for p in paths]
        results = []
        if dev:
            def on(i, rec, row):
                results.append(finish_pose_record(rec, row, names[i]))
        else:
            def on(i, rec):
                results.append(finish_record(rec, names[i], KP3D, K, LEFT))
        for rep in range(2):                       # the first pass captures the graphs and warms the loader
            ld = FrameLoader(paths, threads=8, depth=max(16, 2 * streams * batch + 8))
            results.clear()
            t = time.perf_counter()
            n = runner.run(ld, on)
            dt = time.perf_counter() - t
            ld.close()
        assert n == len(paths) == len(results)
        out[name] = round(n / dt, 1)
        del runner
    return out


def main():
    kernel_only = "--kernel-only" in sys.argv
    recs = records(28)
    res = {"what": "device pose tail (decode + pPose-NMS + pruning + PnP), one MI355X", "left_number": LEFT}
    for B in (1, 28):
        ms, rows = tail_ms(recs, B)
        res["tail_kernel_ms_batch%d" % B] = round(ms, 4)
    if kernel_only:
        print(json.dumps(res))
        return
    res["frames_with_pose_in_sample"] = int((rows[:, 0] == 0).sum())
    h, d = host_us(recs, rows)
    res["host_finish_record_us_per_frame"] = round(h, 1)
    res["finish_pose_record_us_per_frame"] = round(d, 1)
    res["lone_frame_ms"] = lone_frame_ms()
    from PIL import Image
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, fr in enumerate(synth.synth_frames(224, 777)):
            p = os.path.join(tmp, "%04d.png" % i)
            Image.fromarray(fr[:, :, ::-1].copy()).save(p, compress_level=1)
            paths.append(p)
        res["streamed_fps_bf16x3_s4_b1"] = streamed_fps(paths[:112], "bf16x3", 4, 1)
        res["streamed_fps_f16_s3_b28"] = streamed_fps(paths, "f16", 3, 28)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
