#!/usr/bin/env python3
"""Cost of the detector validation tail at the workload's size: B = 64 images of 10 647 rows (416 x 416, heads of 13, 26
and 52 cells a side, 3 anchors, 1 class).

    python tools/bench_yolo_map.py [--batch 64] [--repeat 20] [--out profiles/yolo_map_bench.json]

Measured: bp_yolo_detections with 64, 512 and 4 096 candidates per image (boxes in overlapping clusters, so the greedy
sweep has live and suppressed entries) against its host twin; bp_detector_map_match on the 512-candidate list with four
labels per image; bp_detector_map_reduce at D = 100 000 records, 1 class, 20 000 truths; and the detector's forward
(yolov3-single, random weights, bf16x3) next to the tail of one batch at 512 candidates, which gives the tail's share.
The device entry points are timed with device events around calls on tensors that are already on the device (no
copies and no allocation inside the window), after a warm-up call of the same shape: the median of --repeat with the
spread (min, max).  The host twins are timed with a host clock, --host_repeat times.  Without a GPU the tool fails:
there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from betapose_amd import _lib, yolo_map as M  # noqa: E402

NET = (416, 416)
SHAPES = [(3, 13, 13), (3, 26, 26), (3, 52, 52)]
ROWS = sum(n * h * w for n, h, w in SHAPES)


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


def make_pred(rng, B, cands):
    pred = np.empty((B, ROWS, 6), np.float32)
    for b in range(B):
        centers = rng.uniform(40, 376, (40, 2))
        pred[b, :, 0:2] = centers[rng.integers(0, 40, ROWS)] + rng.normal(0, 14, (ROWS, 2))
        pred[b, :, 2:4] = rng.uniform(30, 90, (ROWS, 2))
        obj = rng.uniform(0.0, 0.004, ROWS)
        obj[rng.permutation(ROWS)[:cands]] = rng.uniform(0.05, 1.0, cands)
        pred[b, :, 4], pred[b, :, 5] = obj, rng.uniform(0.3, 1.0, ROWS)
    return pred


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default=64, type=int)
    ap.add_argument("--repeat", default=20, type=int)
    ap.add_argument("--host_repeat", default=3, type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolo_map_bench.json"))
    args = ap.parse_args(argv)
    import torch
    _lib.require_gpu()
    L, dev, B = _lib.lib(), torch.device("cuda:0"), args.batch
    st = lambda: torch.cuda.current_stream(dev).cuda_stream
    heads = M.heads_table(SHAPES)
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "batch": B, "rows": ROWS, "classes": 1,
           "repeat": args.repeat, "detections": {}}
    keep = {}
    for cands, max_dets in ((64, 1024), (512, 1024), (4096, 4096)):
        pred = make_pred(rng, B, cands)
        d_pred = torch.from_numpy(pred).to(dev)
        dets = torch.empty((B, max_dets, 7), dtype=torch.float32, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        scratch = torch.empty((int(L.bp_yolo_detections_scratch(B, max_dets, 1)) // 4,), dtype=torch.float32, device=dev)
        call = lambda d_pred=d_pred, dets=dets, count=count, scratch=scratch, max_dets=max_dets: _lib.check(L.bp_yolo_detections(
            _lib.ptr(d_pred), B, ROWS, 6, _lib.ptr(heads), 3, 416, 416, 1, .005, .45,
                                                       max_dets, _lib.ptr(dets), _lib.ptr(count), _lib.ptr(scratch), st()))
        t = device_time(call, args.repeat)
        h_dets, h_count = np.empty((B, max_dets, 7), np.float32), np.empty(B, np.int32)
        t["host_twin"] = host_time(lambda: _lib.check(L.bp_yolo_detections_host(_lib.ptr(pred), B, ROWS, 6, _lib.ptr(heads), 3, 416, 416,
                                                                                 1, .005, .45, max_dets, _lib.ptr(h_dets),
                                                                                 _lib.ptr(h_count))), args.host_repeat)
        surv = (dets[:, :, 6] > 0).sum(1).float().mean().item()
        t["max_dets"], t["survivors_per_image"] = max_dets, round(surv, 1)
        t["bit_equal_to_host"] = bool(np.array_equal(dets.cpu().numpy(), h_dets) and np.array_equal(count.cpu().numpy(), h_count))
        res["detections"][str(cands)] = t
        if cands == 512:
            keep = dict(d_pred=d_pred, dets=dets, count=count, call=call, h_dets=h_dets, h_count=h_count)

    # call 2 on the 512-candidate list, four labels per image
    Mn = 4 * B
    labels = np.zeros((Mn, 5), np.float32)
    labels[:, 1:3], labels[:, 3:5] = rng.uniform(.2, .8, (Mn, 2)), rng.uniform(.1, .2, (Mn, 2))
    first = (np.arange(B + 1) * 4).astype(np.int32)
    d_l, d_f = torch.from_numpy(labels).to(dev), torch.from_numpy(first).to(dev)
    stride = 1024
    rec, rc = torch.empty((B, stride, 6), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    tcc, ist = torch.zeros((1,), dtype=torch.int32, device=dev), torch.empty((B, 3), dtype=torch.float64, device=dev)
    claim = torch.empty((Mn + 1,), dtype=torch.int32, device=dev)
    match = lambda: _lib.check(L.bp_detector_map_match(_lib.ptr(keep["dets"]), _lib.ptr(keep["count"]), B, 1024, 1, _lib.ptr(d_l), Mn,
                                                       _lib.ptr(d_f), .5, .25, 0, 0, stride, _lib.ptr(rec), _lib.ptr(rc), _lib.ptr(tcc),
                                                       _lib.ptr(ist), _lib.ptr(claim), st()))
    res["match"] = device_time(match, args.repeat)
    h_rec, h_rc, h_tcc, h_ist = np.empty((B, stride, 6), np.float32), np.empty(B, np.int32), np.zeros(1, np.int32), np.empty((B, 3))
    res["match"]["host_twin"] = host_time(lambda: _lib.check(L.bp_detector_map_match_host(
        _lib.ptr(keep["h_dets"]), _lib.ptr(keep["h_count"]), B, 1024, 1, _lib.ptr(labels), Mn, _lib.ptr(first), .5, .25, 0, 0, stride,
        _lib.ptr(h_rec), _lib.ptr(h_rc), _lib.ptr(h_tcc), _lib.ptr(h_ist))), args.host_repeat)
    res["match"]["records"] = int(rc.sum().item())

    # call 3 at D = 100 000
    D, U, N = 100000, 20000, 5000
    r = np.zeros((D, 6), np.float32)
    r[:, 0] = rng.uniform(.005, 1, D).astype(np.float32)
    img = np.sort(rng.integers(0, N, D)).astype(np.int32)
    r[:, 1], r[:, 2] = img.view(np.float32), 0
    r[:, 3] = np.where(rng.random(D) < .3, rng.integers(0, U, D), -1).astype(np.int32).view(np.float32)
    r[:, 5] = np.arange(D, dtype=np.int32).view(np.float32)
    tc, stats_in = np.array([U], np.int32), rng.uniform(0, 3, (N, 3))
    d_r, d_tc, d_si = torch.from_numpy(r).to(dev), torch.from_numpy(tc).to(dev), torch.from_numpy(stats_in).to(dev)
    apd, sd = torch.empty((1,), dtype=torch.float64, device=dev), torch.empty((8,), dtype=torch.float64, device=dev)
    scr = torch.empty((int(L.bp_detector_map_reduce_scratch(D, U)) // 8 + 1,), dtype=torch.int64, device=dev)
    red = lambda: _lib.check(L.bp_detector_map_reduce(_lib.ptr(d_r), D, _lib.ptr(d_tc), 1, U, _lib.ptr(d_si), N, _lib.ptr(apd),
                                                      _lib.ptr(sd), None, _lib.ptr(scr), st()))
    res["reduce"] = device_time(red, args.repeat)
    aph, sh = np.empty(1), np.empty(8)
    res["reduce"]["host_twin"] = host_time(lambda: _lib.check(L.bp_detector_map_reduce_host(
        _lib.ptr(r), D, _lib.ptr(tc), 1, U, _lib.ptr(stats_in), N, _lib.ptr(aph), _lib.ptr(sh), None)), args.host_repeat)
    res["reduce"].update(D=D, truths=U, images=N, bit_equal_to_host=bool(apd.cpu().numpy()[0] == aph[0] and np.array_equal(sd.cpu().numpy(), sh)))

    # the forward next to the tail (512 candidates)
    from betapose_amd.cfg import yolov3_single_cfg_text
    from betapose_amd.darknet import Darknet
    from betapose_amd.weights import darknet_stream_size
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "net.cfg")
        open(cfg, "w").write(yolov3_single_cfg_text(classes=1))
        net = Darknet(cfg, reso=416, max_batch=B)
        need = darknet_stream_size([b for b in net.blocks if b["type"] != "net"])
        net.load_stream((np.random.default_rng(1).standard_normal(need) * 0.02).astype(np.float32)).cuda()
        net.set_precision("bf16x3")
        x = torch.rand((B, 3, 416, 416), device=dev)
        res["forward"] = device_time(lambda: net(x), max(args.repeat // 4, 3))
    tail = device_time(lambda: (keep["call"](), match()), args.repeat)
    res["tail_512"] = tail
    res["tail_share_of_batch"] = round(tail["median_ms"] / (tail["median_ms"] + res["forward"]["median_ms"]), 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
