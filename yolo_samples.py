#!/usr/bin/env python3
"""Detector training batches -- the counterpart of one ``load_data_detection`` call of the reference's vendored Darknet
(``3_6Dpose_estimator/train_YOLO/src/data.c``), fed by the annotator's ``labels/<frame>.txt`` files:

    python yolo_samples.py --list all.txt --cfg yolov3-single.cfg --batch 64 --out batch.npz
                           [--eval] [--seed 0] [--device cuda:0] [--width 416 --height 416] [--max_boxes 90]

The first batch of the list (shuffled with --seed unless --eval) is built by betapose_amd.yolo_train.YoloSampleLoader
and written to --out: ``inps`` [B, 3, net_h, net_w], ``truth`` [B, max_boxes, 5] = (x, y, w, h, id), ``kept`` [B], the list
indices ``ids`` and the draws (``crop``, ``geom``, ``flip``, ``hsv`` -- zeros, ones in evaluation mode --, ``swap``).  The
network size comes from the cfg's [net] block unless given, the class count and the jitter from its first [yolo] block.
The archive carries fixed time stamps: the same seed gives the same bytes.  Without --device everything runs on the
host twins; no GPU is needed.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from betapose_amd import yolo_train as Y  # noqa: E402
from betapose_amd.cfg import parse_cfg  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="detector training batch")
    p.add_argument("--list", required=True, type=str, help="text file of image paths, one per line (Darknet's train= list)")
    p.add_argument("--cfg", default="yolov3-single.cfg", type=str, help="the detector's cfg")
    p.add_argument("--batch", default=64, type=int, help="samples per batch")
    p.add_argument("--eval", action="store_true", help="evaluation mode: in order, whole frames, no augmentation")
    p.add_argument("--seed", default=0, type=int, help="seed of the shuffle and of every draw")
    p.add_argument("--device", default=None, type=str, help="torch device of the kernels (default: the host twins)")
    p.add_argument("--width", default=0, type=int, help="network input width (default: the cfg's)")
    p.add_argument("--height", default=0, type=int, help="network input height (default: the cfg's)")
    p.add_argument("--max_boxes", default=90, type=int)
    p.add_argument("--out", required=True, type=str, help="the .npz to write")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    blocks = parse_cfg(args.cfg)
    net = blocks[0] if blocks and blocks[0].get("type") == "net" else {}
    heads = Y.yolo_head_params(blocks)
    if not heads:
        raise SystemExit("%s holds no [yolo] block" % args.cfg)
    yolo = [b for b in blocks if b.get("type") == "yolo"][0]
    aug = dict(jitter=float(yolo.get("jitter", .2)), hue=float(net.get("hue", 0)), saturation=float(net.get("saturation", 1)),
               exposure=float(net.get("exposure", 1)))
    size = (args.height or int(net.get("height", 416)), args.width or int(net.get("width", 416)))
    loader = Y.YoloSampleLoader(args.list, args.batch, net_size=size, classes=heads[0]["classes"], max_boxes=args.max_boxes,
                                seed=args.seed, train=not args.eval, device=args.device, **aug)
    it = iter(loader)
    try:
        inps, truth = next(it)
    except StopIteration:
        raise SystemExit("%s names no image" % args.list)
    finally:
        it.close()
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a
    last = loader.last
    B = len(last["ids"])
    hsv = np.tile(np.array([0, 1, 1], np.float32), (B, 1)) if last["hsv"] is None else last["hsv"]
    Y.save_npz(args.out, dict(inps=host(inps), truth=host(truth), kept=host(last["kept"]), ids=last["ids"], crop=last["crop"],
                              geom=last["geom"], flip=last["flip"], hsv=hsv, swap=last["swap"]))
    print("wrote %d samples (%s) to %s" % (B, "eval" if args.eval else "train", args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
