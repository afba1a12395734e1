#!/usr/bin/env python3
"""Key-point detector training -- the counterpart of the reference's ``train_KPD/src/train.py``:

    python train_kpd.py --annot_train annot_train.npz --annot_eval annot_eval.npz --img_folder DIR --out_dir DIR
                        [--nClasses 50] [--LR 1e-3] [--momentum 0] [--weightDecay 0] [--optMethod rmsprop] [--nEpochs 500]
                        [--trainBatch 128] [--validBatch 24] [--loadModel model.pkl] [--addDPG] [--snapshot 5] [--expID default]
                        [--seed 0] [--device cuda:0]

The option names are opt.py's.  ``KPDSampleLoader`` makes the batches (annotate.py's ``annot_*.npz``, the frames under
``--img_folder``); ``TrainableFastPose.train_step`` is one iteration of train() and ``validate_step`` one of valid(), flip
test included.  Per epoch the reference's lines are printed: ``Train-N epoch | loss | acc``, at the epochs where it
validates (``N > 0 and N % 5 == 0``) ``Valid-N epoch`` too, and the best epoch so far.  At those epochs
``<out_dir>/<expID>/model_N.pkl`` -- ``torch.save`` of the state dict, which the reference, weights.load_kpd_pkl and
InferenNet_fast read -- and ``optimizer_N.npz`` are written.  The batches stay on the device from the loader to the
update; the two values read back per iteration are the loss and the accuracy.  ``--device cpu`` runs the host twins.
``--optMethod adam``, DataParallel, TensorBoard and evaluation.py's mAP are out of scope.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser(description="key-point detector training (train_KPD/src/train.py)")
    p.add_argument("--expID", default="default", type=str, help="experiment id: the folder under --out_dir")
    p.add_argument("--snapshot", default=5, type=int, help="accepted as the reference accepts it (its snapshot code is commented out)")
    p.add_argument("--addDPG", default=False, action="store_true", help="train with the DPG window augmentation")
    p.add_argument("--loadModel", default=None, type=str, help="a state-dict .pkl to start from")
    p.add_argument("--nClasses", default=50, type=int, help="number of heat maps")
    p.add_argument("--LR", default=1e-3, type=float)
    p.add_argument("--momentum", default=0, type=float)
    p.add_argument("--weightDecay", default=0, type=float)
    p.add_argument("--optMethod", default="rmsprop", type=str, help="rmsprop (adam is refused)")
    p.add_argument("--nEpochs", default=500, type=int)
    p.add_argument("--trainBatch", default=128, type=int)
    p.add_argument("--validBatch", default=24, type=int)
    p.add_argument("--annot_train", required=True, type=str, help="annotate.py's annot_train.npz")
    p.add_argument("--annot_eval", required=True, type=str, help="annotate.py's annot_eval.npz")
    p.add_argument("--img_folder", required=True, type=str, help="where the annotations' frames lie")
    p.add_argument("--out_dir", default="exp", type=str, help="where <expID>/model_N.pkl goes")
    p.add_argument("--seed", default=0, type=int, help="seed of the shuffle, the augmentation and the initial weights")
    p.add_argument("--device", default="cuda:0", type=str, help="torch device of the kernels, or cpu for the host twins")
    return p


class _Average:
    """DataLogger: the mean weighted by batch size"""

    def __init__(self):
        self.sum, self.cnt = 0.0, 0

    def update(self, value, n):
        self.sum += value * n
        self.cnt += n

    @property
    def avg(self):
        return self.sum / self.cnt if self.cnt else 0.0


def train_kpd(args, out=sys.stdout):
    import numpy as np
    import torch
    from betapose_amd.kpd_train import TrainableFastPose
    from betapose_amd.train_data import KPDSampleLoader
    from betapose_amd.weights import load_kpd_pkl
    dev = None if args.device == "cpu" else args.device
    sd = None
    if args.loadModel:
        print("Loading Model from {}".format(args.loadModel), file=out)
        sd = load_kpd_pkl(args.loadModel)
    else:
        print("Create new model", file=out)
    net = TrainableFastPose(args.nClasses, state_dict=sd, device=dev, seed=args.seed, LR=args.LR, momentum=args.momentum,
                            weightDecay=args.weightDecay, optMethod=args.optMethod)
    folder = os.path.join(args.out_dir, args.expID)
    os.makedirs(folder, exist_ok=True)
    train = KPDSampleLoader(args.annot_train, args.img_folder, args.trainBatch, train=True, seed=args.seed, add_dpg=args.addDPG, device=dev)
    valid = KPDSampleLoader(args.annot_eval, args.img_folder, args.validBatch, train=False, seed=args.seed, device=dev)
    best_acc, best_epoch = 0, 0
    for i in range(args.nEpochs):
        print("############# Starting Epoch {} #############".format(i), file=out)
        loss_log, acc_log = _Average(), _Average()
        for inps, labels, mask in train:
            loss, acc = net.train_step(inps, labels, mask)
            loss_log.update(loss, int(inps.shape[0])), acc_log.update(acc, int(inps.shape[0]))
        print("Train-{idx:d} epoch | loss:{loss:.8f} | acc:{acc:.4f}".format(idx=i, loss=loss_log.avg, acc=acc_log.avg), file=out, flush=True)
        if i > 0 and i % 5 == 0:
            loss_log, acc_log = _Average(), _Average()
            for inps, labels, mask in valid:
                loss, acc = net.validate_step(inps, labels, mask)
                loss_log.update(loss, int(inps.shape[0])), acc_log.update(acc, int(inps.shape[0]))
            torch.save(net.state_dict(), os.path.join(folder, "model_{}.pkl".format(i)))
            np.savez(os.path.join(folder, "optimizer_{}.npz".format(i)), **net.optimizer_state())
            print("Valid-{idx:d} epoch | loss:{loss:.8f} | acc:{acc:.4f}".format(idx=i, loss=loss_log.avg, acc=acc_log.avg), file=out, flush=True)
            if acc_log.avg > best_acc:
                best_epoch, best_acc = i, acc_log.avg
        print("The %d epoch is the best!" % best_epoch, best_acc, file=out, flush=True)
    return net


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        train_kpd(args)
    except ValueError as e:
        raise SystemExit(str(e))
    return 0


if __name__ == "__main__":
    sys.exit(main())
