#!/usr/bin/env python3
"""Cost of one KPD training batch at the reference's size: B = 128 samples from 640 x 480 frames, inputs 320 x 256,
maps 80 x 64, Kp = 50 (``--trainBatch 128``).

    python tools/bench_kpd_samples.py [--batch 128] [--repeat 7] [--no-gpu]

Prints one JSON line.  The host twins are timed with a host clock; the device entry points are timed with device events
around calls on tensors that are already on the device (no copies inside the window), after a warm-up call of the same
shape, best and median of --repeat.  ``loader_step`` is the chain a KPDSampleLoader batch runs on the device
(kpd_targets, kpd_inputs, augment_maps twice) on frames that are already uploaded; the host work of a step (draws,
windows, the frame upload) is reported apart as ``step_host_ms`` and ``upload``.  Bytes are what each call has to move,
computed from the shapes (the input kernel's reads are counted as the window's pixels once), so the rates are lower
bounds on what the memory system delivered; they are call rates (launches included), not kernel rates.  Without a GPU the
device part is "not measured"."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from betapose_amd import _lib, annotate as A, train_data as T  # noqa: E402
from bench_annotate import device_time, host_time, with_rate  # noqa: E402

H, W = 480, 640
INP, RES, KP = (320, 256), (80, 64), 50


def batch(B, seed=3):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    x1, y1 = rng.uniform(150, 330, B), rng.uniform(100, 230, B)
    boxes = np.stack([x1, y1, x1 + rng.uniform(90, 160, B), y1 + rng.uniform(90, 160, B)], axis=1)
    parts = rng.uniform(boxes[:, None, :2] - 5, boxes[:, None, 2:] + 5, (B, KP, 2))
    d = T.draw_augmentation(rng, B)
    ul, br = A.kpd_windows(boxes, d["scale_rate"], (H, W))
    return frames, parts, ul, br, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--no-gpu", action="store_true")
    args = ap.parse_args()
    B = args.batch
    frames, parts, ul, br, d = batch(B)
    idx = np.arange(B, dtype=np.int32)
    blank = np.zeros(B, np.uint8)
    n_inp, n_map = B * 3 * INP[0] * INP[1], B * KP * RES[0] * RES[1]
    win = (np.trunc(br) - np.trunc(ul)).prod(axis=1).sum() * 3          # window pixels read, one byte each
    b_inputs = int(win) + n_inp * 4
    b_aug_inp, b_aug_map = n_inp * 8, n_map * 8                           # one read and one write per element
    b_loss, b_loss_grad = n_map * 12, n_map * 16                          # out, labels, mask (+ grad)
    out = {"batch": B, "frame": [H, W], "input": list(INP), "maps": [KP] + list(RES), "repeat": args.repeat,
           "MB": {"inputs": round(b_inputs / 1e6, 1), "augment_inputs": round(b_aug_inp / 1e6, 1),
                  "augment_maps": round(b_aug_map / 1e6, 1), "loss": round(b_loss / 1e6, 1), "loss_grad": round(b_loss_grad / 1e6, 1)}}

    t0 = time.perf_counter()
    T.draw_augmentation(np.random.default_rng(0), B)
    A.kpd_windows(np.concatenate([ul, br], axis=1), d["scale_rate"], (H, W))
    T.joint_count(parts, ul, br)
    out["step_host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    inp = T.kpd_inputs(frames, idx, ul, br, d["gains"], blank, INP)
    lab, _, mask = A.kpd_targets(parts, ul, br, INP, RES, want_mask=True)
    pred = (lab * np.float32(0.8) + np.random.default_rng(1).normal(0, 0.05, lab.shape).astype(np.float32))
    rep = max(1, args.repeat // 3)
    out["host"] = {"inputs": host_time(lambda: T.kpd_inputs(frames, idx, ul, br, d["gains"], blank, INP), rep),
                   "augment_inputs": host_time(lambda: T.augment_maps(inp, d["flip"], d["angle"]), rep),
                   "augment_maps": host_time(lambda: T.augment_maps(lab, d["flip"], d["angle"]), rep),
                   "loss_grad": host_time(lambda: T.heatmap_loss_accuracy(pred, lab, mask, True), rep)}

    import torch
    if args.no_gpu or not torch.cuda.is_available():
        out["device"] = "not measured"
        print(json.dumps(out))
        return
    lib, ptr, chk = _lib.lib(), _lib.ptr, _lib.check
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pinned = torch.from_numpy(frames).pin_memory()
    d_frames = torch.empty_like(pinned, device=dev)
    d_idx, d_ul, d_br, d_gains, d_blank = up(idx), up(ul), up(br), up(d["gains"]), up(blank)
    d_flip, d_cs = up(d["flip"]), up(T.rotation_terms(d["angle"]))
    d_parts, d_g = up(parts), up(A.gaussian_table(1))
    d_inp, d_inp2 = (torch.empty((B, 3) + INP, dtype=torch.float32, device=dev) for _ in range(2))
    d_lab, d_lab2, d_mask, d_grad = (torch.empty((B, KP) + RES, dtype=torch.float32, device=dev) for _ in range(4))
    d_cen = torch.empty((B, KP, 2), dtype=torch.int32, device=dev)
    d_pred = up(pred)
    d_partial = torch.empty(B * KP, dtype=torch.float64, device=dev)
    d_loss = torch.empty(1, dtype=torch.float64, device=dev)
    d_acc = torch.empty(KP + 1, dtype=torch.float32, device=dev)
    d_p, d_gt = (torch.empty((B, KP, 2), dtype=torch.int32, device=dev) for _ in range(2))
    d_dists = torch.empty((KP, B), dtype=torch.float32, device=dev)

    def upload():
        d_frames.copy_(pinned, non_blocking=True)

    def targets():
        chk(lib.bp_kpd_targets(ptr(d_parts), ptr(d_ul), ptr(d_br), B, KP, INP[0], INP[1], RES[0], RES[1], ptr(d_g), 7, ptr(d_lab),
                               ptr(d_cen), ptr(d_mask), s))

    def inputs():
        chk(lib.bp_kpd_inputs(ptr(d_frames), B, H, W, ptr(d_idx), ptr(d_ul), ptr(d_br), ptr(d_gains), ptr(d_blank), B, INP[0],
                              INP[1], ptr(d_inp), s))

    def aug_inp():
        chk(lib.bp_kpd_augment(ptr(d_inp), B, 3, INP[0], INP[1], ptr(d_flip), ptr(d_cs), None, ptr(d_inp2), s))

    def aug_map():
        chk(lib.bp_kpd_augment(ptr(d_lab), B, KP, RES[0], RES[1], ptr(d_flip), ptr(d_cs), None, ptr(d_lab2), s))

    def loss(grad):
        chk(lib.bp_heatmap_loss_acc(ptr(d_pred), ptr(d_lab), ptr(d_mask), B, KP, RES[0], RES[1], ptr(d_partial), ptr(d_loss),
                                    ptr(d_acc), ptr(d_p), ptr(d_gt), ptr(d_dists), ptr(d_grad) if grad else None, s))

    def step():
        targets(), inputs(), aug_inp(), aug_map()

    upload(), targets()
    torch.cuda.synchronize()
    r = {"name": torch.cuda.get_device_name(0),
         "upload": with_rate(device_time(upload, args.repeat), frames.nbytes),
         "inputs": with_rate(device_time(inputs, args.repeat), b_inputs),
         "augment_inputs": with_rate(device_time(aug_inp, args.repeat), b_aug_inp),
         "augment_maps": with_rate(device_time(aug_map, args.repeat), b_aug_map),
         "loss": with_rate(device_time(lambda: loss(False), args.repeat), b_loss),
         "loss_grad": with_rate(device_time(lambda: loss(True), args.repeat), b_loss_grad),
         "loader_step": with_rate(device_time(step, args.repeat), b_inputs + b_aug_inp + b_aug_map + n_map * 8)}
    loss(True)
    torch.cuda.synchronize()
    want = T.heatmap_loss_accuracy(pred, lab, mask, True)
    same = np.array_equal(d_inp.cpu().numpy().view(np.uint32), inp.view(np.uint32)) and \
        np.array_equal(d_inp2.cpu().numpy().view(np.uint32), T.augment_maps(inp, d["flip"], d["angle"]).view(np.uint32)) and \
        np.array_equal(d_lab2.cpu().numpy().view(np.uint32), T.augment_maps(lab, d["flip"], d["angle"]).view(np.uint32)) and \
        float(d_loss.cpu()[0]) == want[0] and np.array_equal(d_grad.cpu().numpy().view(np.uint32), want[5].view(np.uint32)) and \
        np.array_equal(d_acc.cpu().numpy(), want[1])
    r["equal_to_host"] = bool(same)
    out["device"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
