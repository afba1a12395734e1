#!/usr/bin/env python3
"""Detector training -- the counterpart of the reference's ``./darknet detector train obj.data net.cfg [weights]``
(``3_6Dpose_estimator/train_YOLO/src/detector.c`` train_detector):

    python train_detector.py --data obj.data --cfg net.cfg [--weights w] [--clear] [--max_batches N] [--seed S]
                             [--device cuda:0] [--backup DIR]

The ``train`` list of the ``.data`` file feeds ``YoloSampleLoader`` (Darknet's crop, flip and HSV draws with the cfg's
``jitter``, ``hue``, ``saturation`` and ``exposure``), ``batch / subdivisions`` frames a call; ``TrainableDarknet.train_step``
is one ``train_network_datum``.  After every ``subdivisions`` calls the reference's line is printed: iteration, loss,
the .9 / .1 running average, rate, seconds, images.  ``<backup>/<base>_<i>.weights`` is written when 100 iterations
have passed since the last one, ``<base>_last.weights`` every 100 iterations and ``<base>_final.weights`` at the end;
they load into Darknet, the inference engine and detector_map.py.  The frames stay on the device from the loader to the
update; the one value read back per call is the cost.  ``--device cpu`` runs the host twins.  ``random=1`` (multi-scale
training) is refused: set ``random=0``.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from betapose_amd import yolo_map as M  # noqa: E402
from betapose_amd.darknet_train import TrainableDarknet  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="detector training (Darknet's detector train)")
    p.add_argument("--data", required=True, type=str, help="Darknet's .data file: train, classes, backup")
    p.add_argument("--cfg", required=True, type=str, help="the detector's cfg")
    p.add_argument("--weights", default=None, type=str, help=".weights to start from (their `seen` is kept)")
    p.add_argument("--clear", action="store_true", help="start `seen` at zero")
    p.add_argument("--max_batches", default=None, type=int, help="stop at this iteration instead of the cfg's max_batches")
    p.add_argument("--seed", default=0, type=int, help="seed of the shuffle, the augmentation and the initial weights")
    p.add_argument("--device", default="cuda:0", type=str, help="torch device of the kernels, or cpu for the host twins")
    p.add_argument("--backup", default=None, type=str, help="where the .weights go (default: the .data file's backup)")
    return p


def train_detector(data, cfg, weights=None, clear=False, max_batches=None, seed=0, device="cuda:0", backup=None, out=sys.stdout):
    from betapose_amd.yolo_train import YoloSampleLoader
    opts = M.read_data_cfg(data)
    if "train" not in opts:
        raise ValueError("%s must set 'train'" % data)
    backup = backup or opts.get("backup", "backup")
    os.makedirs(backup, exist_ok=True)
    base = os.path.splitext(os.path.basename(cfg))[0]
    dev = None if device == "cpu" else device
    net = TrainableDarknet(cfg, weights, device=dev, clear=clear, seed=seed)
    o = net.net
    classes = net.heads[0]["head"]["classes"]
    if "classes" in opts and int(opts["classes"]) != classes:
        raise ValueError("%s names %s classes, the cfg's [yolo] blocks %d" % (data, opts["classes"], classes))
    limit = o["max_batches"] if max_batches is None else max_batches
    imgs = o["batch"] * o["subdivisions"]
    batch_num = lambda: net.seen // imgs
    loader = YoloSampleLoader(opts["train"], o["batch"], net_size=(o["height"], o["width"]), classes=classes, seed=seed, train=True,
                              device=dev, jitter=o["jitter"], hue=o["hue"], saturation=o["saturation"], exposure=o["exposure"])
    avg, saved, calls, total, t0 = -1.0, batch_num(), 0, 0.0, time.time()
    save = lambda tag: net.save_weights(os.path.join(backup, "%s_%s.weights" % (base, tag)))
    while batch_num() < limit:
        for inps, truth in loader:      # one pass over the shuffled list; the next pass draws a new order
            if int(inps.shape[0]) != o["batch"]:
                continue                # (the list's remainder: a Darknet batch is always full)
            total += net.train_step(inps, truth)
            calls += 1
            if calls % o["subdivisions"]:
                continue
            loss = total / (o["subdivisions"] * o["batch"])     # train_network: the calls' costs over n * batch
            avg = loss if avg < 0 or avg != avg else avg
            avg = avg * .9 + loss * .1
            i = batch_num()
            print("\n %d: %f, %f avg loss, %f rate, %f seconds, %d images" % (i, loss, avg, net.current_rate(), time.time() - t0,
                                                                              i * imgs), file=out, flush=True)
            total, t0 = 0.0, time.time()
            if i % 100 == 0:
                save("last")
            if i >= saved + 100:
                saved = i
                save("%d" % i)
            if i >= limit:
                break
    save("final")
    return net


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        train_detector(args.data, args.cfg, args.weights, args.clear, args.max_batches, args.seed, args.device, args.backup)
    except ValueError as e:
        raise SystemExit(str(e))
    return 0


if __name__ == "__main__":
    sys.exit(main())
