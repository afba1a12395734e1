#!/usr/bin/env python3
"""Generate tests/golden/kpd_train.npz by running the REFERENCE's own classes under torch CPU autograd (build container
only, like tools/make_golden_kpd_samples.py; nothing of the reference is copied: its ``train_KPD/src/models/layers``
``Bottleneck``, ``SEResnet.make_layer`` / ``forward``, ``SELayer`` and ``DUC`` and ``utils/eval.py``'s heatmapAccuracy are
imported in place).

A tiny FastPose_SE is composed from those classes (stem 4, stages (planes, blocks, stride) = (2, 1, 1), (2, 1, 2),
(2, 2, 1), (4, 1, 2), 2 classes: about 2 900 parameters; the third stage keeps the shape, so make_layer gives it neither
a downsample nor an SE gate; 24 x 20 inputs, batch 4, so the channel maps hold 120, 30, 9, 4, 16, 64 and 256 values) and trained with ``torch.optim.RMSprop`` in float32 as train() does, for two settings: opt.py's
defaults, and ``momentum = 0.9, weightDecay = 1e-4``.  Three consecutive iterations each, from one initial state:

  init.P                      the state before iteration 0 (V and B are zero), every vector in ``keys`` order
  s<k>.i<n>.out, .loss, .acc  the heat maps, MSELoss(out * setMask, labels) and accuracy()[0] of iteration n
  s<k>.i<n>.grad              every parameter's gradient
  s<k>.i<n>.P / .V / .B       the state after the iteration (parameters with running statistics, square_avg, momentum
                              buffer), which is the state before the next
  full_state_dict             keys, shapes and dtypes of the reference's FastPose_SE().state_dict() (50 classes), as JSON
  valid.*                     one valid() batch from the state after setting 0: loss, accuracy and the averaged maps
  err.<quantity>              ref_err = max|float32 - float64| / max|float64| per tensor (a vector in ``keys`` order for
                              the per-parameter quantities), the float64 run starting from the same float32 state; the
                              float64 optimiser step is fed the float32 gradients (a free-running comparison of RMSprop
                              is meaningless: g / (sqrt(v) + eps) is sign-like on the first steps)

The inputs are multiples of 1 / 32 stored as int8 and the labels multiples of 1 / 255 stored as uint8, so the archive
stays small; both sides decode them alike.

Conditions asserted, re-seeding until the reference alone meets them, no quantity exempt: no pre-ReLU value within 1e-5
of zero, no max-pool window with a positive maximum whose two largest values lie within 1e-5, every gradient ref_err <= 2e-3.

The archive is written with fixed time stamps: running this twice gives the same bytes.

Usage: python tools/make_golden_kpd_train.py
"""
from __future__ import annotations

import copy
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import ref_shims  # noqa: E402  (only for where the reference lies)

SRC = os.path.join(ref_shims.REF, "train_KPD", "src")
OUT = os.path.join(ROOT, "tests", "golden", "kpd_train.npz")
STEM, STAGES, NCLS = 4, ((2, 1, 1), (2, 1, 2), (2, 2, 1), (4, 1, 2)), 2
B, H, W = 4, 24, 20
FLIP_PAIRS = ((1, 2),)
SETTINGS = (dict(LR=1e-3, momentum=0.0, weightDecay=0.0), dict(LR=1e-3, momentum=0.9, weightDecay=1e-4))
ITERS = 3
NEAR = 1e-5


def import_reference(out_h):
    sys.dont_write_bytecode = True
    ref_shims._stub("opt", opt=types.SimpleNamespace(outputResH=out_h, nStack=1, nClasses=NCLS))
    for name in ("cv2", "scipy.misc", "torchsample", "torchsample.transforms"):
        if name not in sys.modules:
            ref_shims._stub(name)
    pc = ref_shims._stub("pycocotools")
    pc.coco = ref_shims._stub("pycocotools.coco", COCO=object)
    pc.cocoeval = ref_shims._stub("pycocotools.cocoeval", COCOeval=object)
    sys.path.insert(0, SRC)
    import models.layers.SE_Resnet as R
    import models.layers.DUC as D
    import utils.eval as E
    return R, D.DUC, E


def full_state_dict():
    """keys, shapes and dtypes of the reference's own FastPose_SE().state_dict() at opt.nClasses = 50"""
    sys.modules["opt"].opt.nClasses = 50
    import models.FastPose as FP
    sd = FP.createModel().state_dict()
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]


class Watch:
    """every pre-ReLU tensor of one forward pass"""

    def __init__(self):
        self.seen = []

    def relu(self, x, inplace=False):
        self.seen.append(x.detach().clone())
        return torch.relu(x)

    def hook(self, mod, args):
        self.seen.append(args[0].detach().clone())

    def nearest(self):
        v = min(float(t.abs().min()) for t in self.seen)
        self.seen = []
        return v


def build(R, DUC, watch):
    class Pre(nn.Module):
        make_layer = R.SEResnet.make_layer
        forward = R.SEResnet.forward

        def __init__(self):
            super().__init__()
            self.inplanes, self.block = STEM, R.Bottleneck
            self.conv1 = nn.Conv2d(3, STEM, kernel_size=7, stride=2, padding=3, bias=False)
            self.bn1 = nn.BatchNorm2d(STEM, eps=1e-5, momentum=0.1, affine=True)
            self.relu = nn.ReLU(inplace=True)
            self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
            for i, (planes, blocks, stride) in enumerate(STAGES, start=1):
                setattr(self, "layer%d" % i, self.make_layer(self.block, planes, blocks, stride))

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            last = 4 * STAGES[-1][0]
            self.preact = Pre()
            self.suffle1 = nn.PixelShuffle(2)
            self.duc1 = DUC(last // 4, last // 2, upscale_factor=2)
            self.duc2 = DUC(last // 8, last // 4, upscale_factor=2)
            self.conv_out = nn.Conv2d(last // 16, NCLS, kernel_size=3, stride=1, padding=1)

        def forward(self, x):       # FastPose_SE.forward
            return self.conv_out(self.duc2(self.duc1(self.suffle1(self.preact(x)))))

    R.F = types.SimpleNamespace(relu=watch.relu)        # Bottleneck's three F.relu calls
    m = Tiny()
    for mod in m.modules():
        if isinstance(mod, nn.ReLU):
            mod.inplace = False
            mod.register_forward_pre_hook(watch.hook)
    return m


def pool_gap(m, x):
    """the smallest distance between the two largest values of a max-pool window whose maximum is positive (a window of
    zeros hands its gradient to a position the ReLU's mask zeroes, whichever it picks)"""
    p = m.preact
    with torch.no_grad():       # (functional: the module's running statistics must not move)
        bn, tr = p.bn1, p.bn1.training
        y = torch.relu(torch.nn.functional.batch_norm(p.conv1(x), None if tr else bn.running_mean, None if tr else bn.running_var,
                                                      bn.weight, bn.bias, training=tr, eps=bn.eps))
    cols = torch.nn.functional.unfold(torch.nn.functional.pad(y, (1, 1, 1, 1), value=-1e30).flatten(0, 1)[:, None], 3, stride=2)
    top = cols.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1])[top[:, 0] > 0].min())


def flat(d, keys):
    return np.concatenate([np.asarray(d[k], dtype=np.float32).reshape(-1) for k in keys])


def rel_err(a32, a64):
    a64 = np.asarray(a64, dtype=np.float64)
    return float(np.abs(np.asarray(a32, dtype=np.float64) - a64).max() / max(float(np.abs(a64).max()), 1e-300))


def batches(rng, n):
    out = []
    for _ in range(n):
        q = rng.integers(-64, 65, (B, 3, H, W)).astype(np.int8)
        lab = np.zeros((B, NCLS, 16, 16), np.uint8)
        mask = np.ones((B, NCLS, 16, 16), np.uint8)
        for b in range(B):
            for c in range(NCLS):
                cy, cx = rng.integers(2, 14, 2)
                yy, xx = np.mgrid[0:16, 0:16]
                lab[b, c] = np.rint(255 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 2.0)).astype(np.uint8)
        mask[rng.integers(0, B), rng.integers(0, NCLS)] = 0        # one channel of one sample masked out, as setMask does
        lab *= mask
        out.append((q, lab, mask))
    return out


def decode(q, lab, mask):
    return (torch.from_numpy(q.astype(np.float32) / np.float32(32)), torch.from_numpy(lab.astype(np.float32) / np.float32(255)),
            torch.from_numpy(mask.astype(np.float32)))


def attempt(seed, R, DUC, E):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    watch = Watch()
    model0 = build(R, DUC, watch)
    sd_keys = list(model0.state_dict().keys())
    keys = [k for k in sd_keys if not k.endswith("num_batches_tracked")]
    pkeys = [k for k, _ in model0.named_parameters()]
    data = batches(rng, ITERS + 1)
    dataset = types.SimpleNamespace(accIdxs=tuple(range(1, NCLS + 1)))
    crit = nn.MSELoss()
    arrays, errs = {}, {}
    sd0 = {k: v.clone() for k, v in model0.state_dict().items()}
    arrays["init.P"] = flat({k: v.numpy() for k, v in sd0.items()}, keys)
    worst_near, worst_gap = np.inf, np.inf
    final = None
    for s, hp in enumerate(SETTINGS):
        m = build(R, DUC, watch)
        m.load_state_dict(sd0)
        m.train()
        opt = torch.optim.RMSprop(m.parameters(), lr=hp["LR"], momentum=hp["momentum"], weight_decay=hp["weightDecay"])
        for it in range(ITERS):
            tag = "s%d.i%d" % (s, it)
            inps, labels, mask = decode(*data[it])
            # the float64 twin starts from the same float32 state, optimiser state included
            m64 = copy.deepcopy(m).double()
            o64 = torch.optim.RMSprop(m64.parameters(), lr=hp["LR"], momentum=hp["momentum"], weight_decay=hp["weightDecay"])
            st = opt.state_dict()
            if st["state"]:
                st = copy.deepcopy(st)
                for v in st["state"].values():
                    for k2 in ("square_avg", "momentum_buffer"):
                        if k2 in v and v[k2] is not None:
                            v[k2] = v[k2].double()
                o64.load_state_dict(st)
            worst_gap = min(worst_gap, pool_gap(m, inps))
            watch.seen = []
            out = m(inps.requires_grad_())
            worst_near = min(worst_near, watch.nearest())
            loss = crit(out.mul(mask), labels)
            acc = E.accuracy(out.data.mul(mask), labels.data, dataset)
            opt.zero_grad()
            loss.backward()
            grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
            opt.step()
            out64 = m64(inps.detach().double())
            watch.seen = []
            loss64 = crit(out64.mul(mask.double()), labels.double())
            o64.zero_grad()
            loss64.backward()
            g64 = {k: p.grad.detach().clone() for k, p in m64.named_parameters()}
            for k, p in m64.named_parameters():
                p.grad = grads[k].double()
            o64.step()
            post = {k: v.detach().numpy() for k, v in m.state_dict().items()}
            post64 = {k: v.detach().numpy() for k, v in m64.state_dict().items()}
            V = {k: opt.state[p]["square_avg"].numpy() for k, p in m.named_parameters()}
            V64 = {k: o64.state[p]["square_avg"].numpy() for k, p in m64.named_parameters()}
            arrays[tag + ".out"] = out.detach().numpy()
            arrays[tag + ".loss"] = np.float64(loss.item())
            arrays[tag + ".acc"] = np.float32(acc[0])
            arrays[tag + ".grad"] = flat({k: g.numpy() for k, g in grads.items()}, pkeys)
            arrays[tag + ".P"] = flat(post, keys)
            arrays[tag + ".V"] = flat(V, pkeys)
            errs[tag + ".out"] = rel_err(out.detach().numpy(), out64.detach().numpy())
            errs[tag + ".loss"] = rel_err(loss.item(), loss64.item())
            errs[tag + ".grad"] = [rel_err(grads[k].numpy(), g64[k].numpy()) for k in pkeys]
            # parameters from the float64 step fed the float32 gradients; running statistics from the float64 forward pass
            errs[tag + ".P"] = [rel_err(post[k], post64[k]) for k in keys]
            errs[tag + ".V"] = [rel_err(V[k], V64[k]) for k in pkeys]
            if hp["momentum"] > 0:
                Bf = {k: opt.state[p]["momentum_buffer"].numpy() for k, p in m.named_parameters()}
                B64 = {k: o64.state[p]["momentum_buffer"].numpy() for k, p in m64.named_parameters()}
                arrays[tag + ".B"] = flat(Bf, pkeys)
                errs[tag + ".B"] = [rel_err(Bf[k], B64[k]) for k in pkeys]
        if s == 0:
            final = {k: v.clone() for k, v in m.state_dict().items()}
    # valid(): one batch from the state after setting 0
    m = build(R, DUC, watch)
    m.load_state_dict(final)
    m.eval()
    m64 = copy.deepcopy(m).double()
    inps, labels, mask = decode(*data[ITERS])

    def valid(mod, x, lab, msk):
        with torch.no_grad():
            out = mod(x)
            loss = crit(out.mul(msk), lab)
            f = torch.flip(mod(torch.flip(x, [3])), [3])            # flip_v
            for a, b in FLIP_PAIRS:                                 # shuffleLR_v
                f[:, [a - 1, b - 1]] = f[:, [b - 1, a - 1]]
            return loss, (f + out) / 2

    worst_gap = min(worst_gap, pool_gap(m, inps), pool_gap(m, torch.flip(inps, [3])))
    watch.seen = []
    loss, avg = valid(m, inps, labels, mask)
    worst_near = min(worst_near, watch.nearest())
    loss64, avg64 = valid(m64, inps.double(), labels.double(), mask.double())
    acc = E.accuracy(avg.mul(mask), labels, dataset)
    arrays["valid.loss"], arrays["valid.acc"], arrays["valid.maps"] = np.float64(loss.item()), np.float32(acc[0]), avg.numpy()
    arrays["valid.acc_all"] = acc.numpy().astype(np.float32)
    errs["valid.loss"], errs["valid.maps"] = rel_err(loss.item(), loss64.item()), rel_err(avg.numpy(), avg64.numpy())
    worst_grad = max(max(v) for k, v in errs.items() if k.endswith(".grad"))
    ok = worst_near > NEAR and worst_gap > NEAR and worst_grad <= 2e-3
    print("seed %d: nearest pre-ReLU %.3g, pool gap %.3g, worst gradient ref_err %.3g -> %s"
          % (seed, worst_near, worst_gap, worst_grad, "ok" if ok else "redraw"))
    if not ok:
        return None
    for i, (q, lab, msk) in enumerate(data):
        arrays["batch%d.inps_q" % i], arrays["batch%d.labels_q" % i], arrays["batch%d.mask" % i] = q, lab, msk
    for k, v in errs.items():
        arrays["err." + k] = np.asarray(v, dtype=np.float64)
    sd = model0.state_dict()
    arrays["full_state_dict"] = np.frombuffer(json.dumps(full_state_dict()).encode(), dtype=np.uint8)
    arrays["meta"] = np.frombuffer(json.dumps(dict(
        stem=STEM, stages=STAGES, n_classes=NCLS, batch=B, height=H, width=W, flip_pairs=FLIP_PAIRS, settings=SETTINGS, iters=ITERS,
        seed=seed, keys=keys, param_keys=pkeys, shapes={k: list(sd[k].shape) for k in sd_keys},
        state_dict=[[k, list(sd[k].shape), str(sd[k].dtype).replace("torch.", "")] for k in sd_keys],
        worst=dict(near=worst_near, pool_gap=worst_gap, grad_ref_err=worst_grad)), sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def main():
    from betapose_amd.train_data import save_npz
    R, DUC, E = import_reference(16)
    for seed in range(100, 200):
        arrays = attempt(seed, R, DUC, E)
        if arrays is not None:
            save_npz(OUT, arrays)
            print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))
            for k in sorted(arrays):
                if k.startswith("err."):
                    print("  %-16s %.3g" % (k[4:], float(np.max(arrays[k]))))
            return
    raise SystemExit("no seed met the conditions")


if __name__ == "__main__":
    main()
