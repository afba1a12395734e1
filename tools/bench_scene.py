#!/usr/bin/env python3
"""Shared multi-class detector against one detector per object, K = 8 synthetic objects, bf16x3, device
pose tail on, one GPU.  One JSON line; ``--out FILE`` also writes it there (profiles/scene_bench.json):

  * ms per frame of ONE ``ScenePipeline`` (resize + 15-class detector once, eight key-point chains) against the SUM of the
    eight per-object ``FramePipeline`` graphs it replaces (each: resize + its single-class detector + its chain), the two
    alternating on one stream: HIP events around each, median of 20 after a warm-up, with the samples' spread;
  * (frame, object) units per second of ``MultiObjectRunner`` in both modes at 4 streams over written PNGs, second pass.

The baseline is the per-object runner as it stands.  ``shared_not_slower`` is the one condition: the shared median may
exceed the per-object median by no more than the larger of the two samples' spreads (max - min).

    python tools/bench_scene.py [--out profiles/scene_bench.json] [--frames 48]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from betapose_amd import cfg as C, synth  # noqa: E402
from betapose_amd.darknet import Darknet  # noqa: E402
from betapose_amd.kpd import FastPoseHIP  # noqa: E402
from betapose_amd.pipeline import FramePipeline, MultiObjectRunner, ScenePipeline, frame_sharded_owner  # noqa: E402
from betapose_amd.weights import fastpose_stream_from_state_dict  # noqa: E402

OBJS = [1, 5, 6, 8, 9, 10, 11, 12]                  # the eight Occlusion-LineMod objects
CLASS_OF = {o: o - 1 for o in OBJS}
MODE, LEFT, STREAMS, REPS, WARM = "bf16x3", 10, 4, 20, 5


def det_single(obj):
    d = Darknet("yolo/cfg/yolov3-single.cfg", reso=416).load_stream(synth.synth_yolo_stream(synth.object_seeds(obj)[0])).cuda()
    d.set_precision(MODE)
    return d


def det_shared():
    d = Darknet("yolo/cfg/yolov3-single.cfg", reso=416)
    d.blocks = C.parse_cfg_text(C.yolov3_single_cfg_text(classes=15))
    d.net_info = d.blocks[0]
    d.load_stream(synth.synth_yolo_stream(1, d.blocks)).cuda()
    d.set_precision(MODE)
    return d


def pose_net(obj):
    sd = synth.synth_fastpose_state_dict(synth.object_seeds(obj)[1], 50)
    p = FastPoseHIP.from_stream(fastpose_stream_from_state_dict(sd, 50), n_classes=50).cuda()
    p.set_precision(MODE)
    return p


def solver(obj):
    return (synth.synth_kp3d(50, seed=7 + obj), synth.CAM_K, LEFT)


def stats(ts):
    ts = np.asarray(ts)
    return {"median": round(float(np.median(ts)), 4), "min": round(float(ts.min()), 4), "max": round(float(ts.max()), 4),
            "spread": round(float(ts.max() - ts.min()), 4)}


def frame_ms(det15, dets, poses):
    """One frame on one stream: the scene graph against the eight per-object graphs back to back, alternating."""
    frame = torch.from_numpy(synth.synth_frame(99)).cuda().unsqueeze(0)
    scene = ScenePipeline(det15, poses, CLASS_OF, 480, 640, frames=frame)
    pipes = []
    for o in OBJS:
        scene.set_pose_solver(o, *solver(o))
        fp = FramePipeline(dets[o], poses[o], 480, 640, batch=1, frames=frame)
        fp.set_pose_solver(*solver(o))
        pipes.append(fp.prepare())
    scene.prepare()

    def shared():
        scene.enqueue()

    def per_object():
        for fp in pipes:
            fp.enqueue()
    ts = {"shared": [], "per_object": []}
    for i in range(WARM + REPS):
        for name, fn in (("shared", shared), ("per_object", per_object)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= WARM:
                ts[name].append(e0.elapsed_time(e1))
    counts = {"shared": scene.kernel_count(), "per_object": sum(fp.kernel_count() for fp in pipes)}
    detected = int((scene.results.cpu()[:, 0].contiguous().view(torch.int32) >= 0).sum())
    return {k: stats(v) for k, v in ts.items()}, counts, detected


def runner_units_per_s(det15, dets, poses, paths):
    from betapose_amd.frame_loader import FrameLoader
    K, n = len(OBJS), len(paths)
    solvers = {o: solver(o) for o in OBJS}
    out = {}
    for name in ("per_object", "shared"):
        if name == "shared":
            runner = MultiObjectRunner(poses, OBJS, 480, 640, streams=STREAMS, pose_solvers=solvers, shared_detector=(det15, CLASS_OF))
            owner = frame_sharded_owner(K, 1)
        else:
            runner = MultiObjectRunner({o: (dets[o], poses[o]) for o in OBJS}, OBJS, 480, 640, streams=STREAMS, pose_solvers=solvers)
            owner = lambda u: 0   # noqa: E731
        for rep in range(2):                           # the first pass captures the graphs and warms the loader
            ld = FrameLoader(paths, threads=8, depth=max(16, 2 * STREAMS + 8))
            seen = []
            t = time.perf_counter()
            units = runner.run(ld, list(range(n)), lambda u: owner(u) == 0, lambda u, rec, pose: seen.append(u))
            dt = time.perf_counter() - t               # the runner returns after the last record reached the host
            ld.close()
        assert units == n * K == len(seen)
        out[name] = {"units_per_s": round(units / dt, 1), "frames_per_s": round(n / dt, 1)}
        del runner
    return out


def main():
    n_frames = int(sys.argv[sys.argv.index("--frames") + 1]) if "--frames" in sys.argv else 48
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_scene.py needs a GPU")
    det15, dets, poses = det_shared(), {o: det_single(o) for o in OBJS}, {o: pose_net(o) for o in OBJS}
    ms, counts, detected = frame_ms(det15, dets, poses)
    res = {"what": "one shared 15-class detector pass + 8 key-point chains against 8 per-object pipelines, one MI355X",
           "objects": OBJS, "precision": MODE, "pose_tail": "device, left_number %d" % LEFT, "samples": REPS,
           "frame_ms": ms, "graph_nodes_per_frame": counts, "classes_detected_in_sample_frame": detected}
    noise = max(ms["shared"]["spread"], ms["per_object"]["spread"])
    res["per_object_over_shared_ms"] = round(ms["per_object"]["median"] / ms["shared"]["median"], 3)
    res["noise_ms"] = noise
    res["shared_not_slower"] = bool(ms["shared"]["median"] <= ms["per_object"]["median"] + noise)
    from PIL import Image
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, fr in enumerate(synth.synth_frames(n_frames, 777)):
            p = os.path.join(tmp, "%04d.png" % i)
            Image.fromarray(fr[:, :, ::-1].copy()).save(p, compress_level=1)
            paths.append(p)
        res["runner_%d_streams" % STREAMS] = runner_units_per_s(det15, dets, poses, paths)
    r = res["runner_%d_streams" % STREAMS]
    res["shared_over_per_object_units_per_s"] = round(r["shared"]["units_per_s"] / r["per_object"]["units_per_s"], 3)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
