#!/usr/bin/env python3
"""KPD training batches -- the counterpart of one step of the reference's ``train_KPD/src`` data loader
(``utils/dataset/coco.py`` + ``utils/pose.py`` generateSampleBox), fed by the annotator's output:

    python kpd_samples.py --annot <out>/annot_train.npz --img_folder <frames> --batch 32 --out batch.npz
                          [--eval] [--addDPG] [--seed 0] [--device cuda:0] [--inputResH 320 --inputResW 256
                          --outputResH 80 --outputResW 64] [--rotate 40] [--hmGauss 1]

The first batch of the sequence (shuffled with --seed unless --eval) is built by betapose_amd.train_data.KPDSampleLoader
and written to --out: ``inps`` [B, 3, inpH, inpW], ``labels`` and ``setMask`` [B, Kp, resH, resW], the windows ``ul`` /
``br``, ``joint_num``, the annotation indices ``ids`` and the draws (``gains`` -- ones in evaluation mode --,
``scale_rate``, ``flip``, ``angle``).  The archive carries fixed time stamps: the same seed gives the same bytes.
Without --device everything runs on the host twins; no GPU is needed.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from betapose_amd import train_data as T  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="KPD training batch")
    p.add_argument("--annot", required=True, type=str, help="annot_train.npz / annot_eval.npz of annotate.py")
    p.add_argument("--img_folder", required=True, type=str, help="folder of the frames the annotations name")
    p.add_argument("--batch", default=32, type=int, help="samples per batch (the reference's --trainBatch)")
    p.add_argument("--eval", action="store_true", help="evaluation mode: in order, no augmentation")
    p.add_argument("--addDPG", action="store_true", help="the reference's --addDPG window jitter")
    p.add_argument("--seed", default=0, type=int, help="seed of the shuffle and of every draw")
    p.add_argument("--device", default=None, type=str, help="torch device of the kernels (default: the host twins)")
    p.add_argument("--inputResH", default=320, type=int)
    p.add_argument("--inputResW", default=256, type=int)
    p.add_argument("--outputResH", default=80, type=int)
    p.add_argument("--outputResW", default=64, type=int)
    p.add_argument("--rotate", default=40, type=float, help="degree of rotation augmentation")
    p.add_argument("--hmGauss", default=1, type=int, help="heat-map Gaussian size")
    p.add_argument("--out", required=True, type=str, help="the .npz to write")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    loader = T.KPDSampleLoader(args.annot, args.img_folder, args.batch, train=not args.eval, seed=args.seed, add_dpg=args.addDPG,
                               device=args.device, in_res=(args.inputResH, args.inputResW),
                               out_res=(args.outputResH, args.outputResW), sigma=args.hmGauss, rotate=args.rotate)
    it = iter(loader)
    try:
        inps, labels, mask = next(it)
    except StopIteration:
        raise SystemExit("%s holds no annotation" % args.annot)
    finally:
        it.close()
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a
    last = loader.last
    B = len(last["ids"])
    gains = np.ones((B, 3), np.float32) if last["gains"] is None else last["gains"]
    T.save_npz(args.out, dict(inps=host(inps), labels=host(labels), setMask=host(mask), ul=last["ul"], br=last["br"],
                              joint_num=last["joint_num"], ids=last["ids"], gains=gains, scale_rate=last["scale_rate"],
                              flip=last["flip"], angle=last["angle"]))
    print("wrote %d samples (%s%s) to %s" % (B, "eval" if args.eval else "train", ", addDPG" if args.addDPG else "", args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
