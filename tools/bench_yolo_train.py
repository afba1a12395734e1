#!/usr/bin/env python3
"""Cost of one detector training batch at the workload's size: B = 64 frames of 640 x 480 resized to 416 x 416, the
truth rows, and the yolo-layer loss of the three heads (13, 26 and 52 cells a side, 3 anchors, 1 class) with 1 and 8
truths per image.

    python tools/bench_yolo_train.py [--batch 64] [--repeat 20] [--out profiles/yolo_train_bench.json]

Writes the JSON to --out and prints it.  The device entry points are timed with device events around calls on tensors
that are already on the device (no copies inside the window), after a warm-up call of the same shape: the median of
--repeat with the spread (min, max).  Bytes are what each call has to move, computed from the shapes: for the inputs
the float32 written (B x 3 x 416 x 416 x 4) plus the taps read, counted as each crop's frame pixels once (3 bytes each);
for a loss the head read once and delta and act written once, plus delta read once more by the cost step.  The rate is
set against the 6.3 TB/s a copy reaches on an MI355X; it is a call rate (launches and the argument read-back included),
not a kernel rate.  The host twins are timed with a host clock.  Without a GPU the tool fails: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from betapose_amd import _lib, yolo_train as Y  # noqa: E402

H, W, NET = 480, 640, (416, 416)
ANCHORS = np.array([10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326], np.float32).reshape(9, 2)
HEADS = ((13, (6, 7, 8)), (26, (3, 4, 5)), (52, (0, 1, 2)))
COPY_CEILING_TBPS = 6.3


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
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def host_time(fn, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def with_rate(t, nbytes):
    t = dict(t)
    t["MB"] = round(nbytes / 1e6, 2)
    t["TBps_at_median"] = round(nbytes / 1e12 / (t["median_ms"] / 1e3), 3)
    t["share_of_copy_ceiling"] = round(t["TBps_at_median"] / COPY_CEILING_TBPS, 3)
    return t


def truths(rng, B, per_image):
    labels = np.zeros((B * per_image, 5), np.float32)
    a = ANCHORS[rng.integers(0, 9, len(labels))] / NET[0]
    labels[:, 1:3] = rng.uniform(0.2, 0.8, (len(labels), 2))
    labels[:, 3:5] = a * rng.uniform(0.8, 1.2, a.shape)
    first = (np.arange(B + 1) * per_image).astype(np.int32)
    return labels, first, Y.draw_swaps(rng, first)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "yolo_train_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_yolo_train needs an AMD GPU: there is no fallback")
    B = args.batch
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    crop, geom, flip, hsv = Y.draw_detection_augmentation(rng, B, (H, W))
    idx = np.arange(B, dtype=np.int32)
    clipped = (np.minimum(crop[:, 0] + crop[:, 2], W) - np.maximum(crop[:, 0], 0)) * (np.minimum(crop[:, 1] + crop[:, 3], H) - np.maximum(crop[:, 1], 0))
    b_inputs = B * 3 * NET[0] * NET[1] * 4 + int(clipped.sum()) * 3
    out = {"batch": B, "frame": [H, W], "net": list(NET), "repeat": args.repeat, "copy_ceiling_TBps": COPY_CEILING_TBPS}

    lib, ptr, chk = _lib.lib(), _lib.ptr, _lib.check
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_frames, d_idx, d_crop, d_flip, d_hsv, d_geom = up(frames), up(idx), up(crop), up(flip), up(hsv), up(geom)
    d_out = torch.empty((B, 3) + NET, dtype=torch.float32, device=dev)

    def inputs():
        chk(lib.bp_yolo_inputs(ptr(d_frames), B, H, W, ptr(d_idx), ptr(d_crop), ptr(d_flip), ptr(d_hsv), B, NET[0], NET[1], ptr(d_out), s))

    r = {"name": torch.cuda.get_device_name(0), "inputs": with_rate(device_time(inputs, args.repeat), b_inputs)}
    host = {"inputs": host_time(lambda: Y.yolo_inputs(frames, idx, crop, flip, hsv, NET), 3)}
    same = np.array_equal(d_out.cpu().numpy().view(np.uint32), Y.yolo_inputs(frames, idx, crop, flip, hsv, NET).view(np.uint32))

    d_anchors = up(ANCHORS)
    for per_image in (1, 8):
        labels, first, swap = truths(rng, B, per_image)
        M = len(labels)
        d_lab, d_first, d_swap = up(labels), up(first), up(swap)
        d_order = torch.empty(M, dtype=torch.int32, device=dev)
        d_truth = torch.empty((B, 90, 5), dtype=torch.float32, device=dev)
        d_kept = torch.empty(B, dtype=torch.int32, device=dev)

        def truth():
            chk(lib.bp_yolo_truth(ptr(d_lab), M, ptr(d_first), ptr(d_swap), ptr(d_geom), ptr(d_flip), B, 1, 90, NET[1], NET[0], 0,
                                  ptr(d_order), ptr(d_truth), ptr(d_kept), s))

        key = "truths_%d" % per_image
        r[key] = {"truth": device_time(truth, args.repeat)}
        h_truth, _ = Y.yolo_truth(labels, first, swap, geom, flip, 1, 90, NET)
        host[key] = {"truth": host_time(lambda: Y.yolo_truth(labels, first, swap, geom, flip, 1, 90, NET), 3)}
        same = same and np.array_equal(d_truth.cpu().numpy().view(np.uint32), h_truth.view(np.uint32))
        for g, mask in HEADS:
            x = rng.normal(0, 1.5, (B, 18, g, g)).astype(np.float32)
            d_x, d_mask = up(x), up(np.array(mask, np.int32))
            d_act, d_delta = torch.empty_like(d_x), torch.empty_like(d_x)
            d_cost, d_stats = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(7, dtype=torch.float64, device=dev)
            d_partial = torch.empty(int(lib.bp_yolo_loss_partials(B, 3, 1, g, g)), dtype=torch.float64, device=dev)

            def loss():
                chk(lib.bp_yolo_loss(ptr(d_x), B, 18, 3, 1, g, g, NET[1], NET[0], ptr(d_anchors), 9, ptr(d_mask), ptr(d_truth), 90, 0.7,
                                     1.0, 0, ptr(d_act), ptr(d_delta), ptr(d_cost), ptr(d_stats), ptr(d_partial), s))

            r[key]["loss_%d" % g] = with_rate(device_time(loss, args.repeat), x.nbytes * 4)
            t0 = time.perf_counter()
            cost, _, delta, _ = Y.yolo_loss(x, h_truth, NET, ANCHORS, mask, 1, 0.7, 1.0)
            host[key]["loss_%d" % g] = {"ms": round((time.perf_counter() - t0) * 1e3, 3)}
            same = same and float(d_cost.cpu()[0]) == cost and np.array_equal(d_delta.cpu().numpy().view(np.uint32), delta.view(np.uint32))
    r["equal_to_host"] = bool(same)
    out["device"], out["host"] = r, host
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
