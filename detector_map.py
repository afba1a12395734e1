#!/usr/bin/env python3
"""Detector validation -- the counterpart of the reference's ``./darknet detector map obj.data net.cfg net.weights``
(``3_6Dpose_estimator/train_YOLO/src/detector.c`` validate_detector_map):

    python detector_map.py --data obj.data --cfg net.cfg --weights net.weights
                           [--thresh .25] [--iou_thresh .5] [--batch 64] [--device cuda:0] [--max_dets 1024]

The ``valid`` list of the ``.data`` file is read ``--batch`` frames at a time: FrameLoader decodes them, ``yolo_inputs``
with the whole-frame crop is Darknet's ``resize_image`` (no letterbox), the engine of ``bp_yolo_create_darknet`` (bf16x3
mode) predicts, and ``DetectorMap.update`` keeps Darknet's box list (every box above 0.005, ``do_nms_sort`` at 0.45) and
matches it to the label files at ``--iou_thresh``.  The report is the reference's: the 11-point AP per class, precision,
recall, F1, TP, FP, FN and average IoU at ``--thresh``, and mAP.  A ``.data`` file that sets ``difficult`` or ``map`` is
refused: both are out of scope.  The network input must be square.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from betapose_amd import yolo_map as M  # noqa: E402
from betapose_amd.cfg import parse_cfg  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="detector validation (Darknet's detector map)")
    p.add_argument("--data", required=True, type=str, help="Darknet's .data file: valid, names, classes")
    p.add_argument("--cfg", required=True, type=str, help="the detector's cfg")
    p.add_argument("--weights", required=True, type=str, help="the detector's .weights")
    p.add_argument("--thresh", default=.25, type=float, help="confidence of the precision / recall / IoU line")
    p.add_argument("--iou_thresh", default=.5, type=float, help="IoU above which a detection matches a label")
    p.add_argument("--batch", default=64, type=int, help="frames per batch")
    p.add_argument("--device", default="cuda:0", type=str, help="torch device of the engine and the kernels")
    p.add_argument("--max_dets", default=1024, type=int, help="candidates per image kept on the device (more: host twin)")
    return p


def read_names(path):
    with open(path) as f:
        return [ln.rstrip("\r\n") for ln in f if ln.strip()]


def detector_map(data, cfg, weights, thresh=.25, iou_thresh=.5, batch=64, device="cuda:0", max_dets=1024, want_pr=False):
    """The whole run: ``(result, names)``, ``result`` as DetectorMap.result() gives it."""
    import torch
    from betapose_amd import _lib
    from betapose_amd.yolo_train import YoloSampleLoader
    opts = M.read_data_cfg(data)
    for key in ("difficult", "map"):
        if key in opts:
            raise ValueError("%s sets '%s', which is not supported (out of scope: DESIGN.md 3.12)" % (data, key))
    if "valid" not in opts or "names" not in opts:
        raise ValueError("%s must set 'valid' and 'names'" % data)
    names = read_names(opts["names"])
    blocks = parse_cfg(cfg)
    net_h, net_w, shapes, classes = M.cfg_heads(blocks)
    if net_h != net_w:
        raise ValueError("the engine takes a square network input, the cfg asks for %d x %d" % (net_w, net_h))
    if "classes" in opts and opts["classes"] != classes:
        raise ValueError("%s names %d classes, the cfg's [yolo] blocks %d" % (data, opts["classes"], classes))
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the detector engine runs on a GPU: --device must be a cuda device")
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    _lib.require_gpu()
    loader = YoloSampleLoader(opts["valid"], batch, net_size=(net_h, net_w), classes=classes, train=False, device=device)
    dm = M.DetectorMap(classes, M.heads_table(shapes), (net_h, net_w), iou_thresh, thresh, max_dets=max_dets, device=device)
    h = C.c_void_p()
    with torch.cuda.device(index):
        _lib.check(_lib.lib().bp_yolo_create_darknet(cfg.encode(), weights.encode(), net_w, int(batch), index, C.byref(h)))
        try:
            _lib.check(_lib.lib().bp_yolo_set_precision(h, 2))      # bf16x3: fp32-accurate
            rows, attrs = _lib.lib().bp_yolo_rows(h), _lib.lib().bp_yolo_attrs(h)
            if attrs != 5 + classes or rows != sum(n * gh * gw for n, gh, gw in shapes):
                raise ValueError("the engine's rows (%d x %d) do not match the cfg's [yolo] blocks" % (rows, attrs))
            for inps, _ in loader:
                x = inps.contiguous()
                pred = torch.empty((x.shape[0], rows, attrs), device=x.device, dtype=torch.float32)
                _lib.check(_lib.lib().bp_yolo_forward(h, x.data_ptr(), x.shape[0], pred.data_ptr(), _lib.current_stream()))
                dm.update(pred, loader.last["labels"], loader.last["first"])
            result = dm.result(want_pr)
            torch.cuda.synchronize(index)
        finally:
            _lib.lib().bp_yolo_destroy(h)
    return result, names


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        result, names = detector_map(args.data, args.cfg, args.weights, args.thresh, args.iou_thresh, args.batch, args.device,
                                     args.max_dets)
    except ValueError as e:
        raise SystemExit(str(e))
    print("\n".join(M.report_lines(result, names)))
    if result["overflow_images"]:
        print("%d image(s) had more than %d candidates and went through the host twin" % (len(result["overflow_images"]), args.max_dets))
    return 0


if __name__ == "__main__":
    sys.exit(main())
