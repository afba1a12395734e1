#!/usr/bin/env python3
"""What one training iteration costs on the device: the YOLOv3 single-class net (the layers of
``yolo-linemod-single.cfg``, random=0) at 416 x 416, net batch 4, through TrainableDarknet.train_step, timed with
device events: the median of ``--steps`` iterations after ``--warmup``, with min and max; the time split by role
(forward GEMM, filter gradient, input gradient, batch norm, update, heads, the rest: shortcut / route / upsample adds
and zeroing); the achieved TFLOP/s of each GEMM role; and the same iteration under torch autograd on the same device.

    python tools/bench_darknet_train.py [--steps 20] [--warmup 3] [--batch 4] [--size 416] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from betapose_amd import cfg as C  # noqa: E402
from betapose_amd.darknet_train import TrainableDarknet  # noqa: E402

ROLES = {0: "forward", 1: "filter_grad", 2: "input_grad"}


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def torch_iteration(torch, net, x, deltas):
    """the same layers under autograd: conv2d, batch_norm with batch statistics, leaky_relu; SGD with momentum"""
    F = torch.nn.functional
    params = []
    for l in net.convs:
        l["_t"] = [l[k].clone().requires_grad_(True) for k in ("weights", "biases") + (("scales",) if l["bn"] else ())]
        params += l["_t"]
    opt = torch.optim.SGD(params, lr=1e-4, momentum=.9, weight_decay=5e-4)

    def step():
        outs, h, heads = [], x, []
        for l in net.layers:
            t = l["type"]
            if t == "convolutional":
                p = l["_t"]
                h = F.conv2d(h, p[0], None if l["bn"] else p[1], l["stride"], l["size"] // 2)
                if l["bn"]:
                    h = F.batch_norm(h, None, None, p[2], p[1], True)
                if l["leaky"]:
                    h = F.leaky_relu(h, .1)
            elif t == "shortcut":
                h = h + outs[l["src"]]
            elif t == "route":
                h = torch.cat([outs[s] for s in l["src"]], 1)
            elif t == "upsample":
                h = F.interpolate(h, scale_factor=2, mode="nearest")
            else:
                heads.append(h)
            outs.append(h)
        opt.zero_grad(set_to_none=True)
        sum((a * d).sum() for a, d in zip(heads, deltas)).backward()
        opt.step()
    return step


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    import torch
    dev = torch.device(args.device)
    text = ("[net]\nbatch=%d\nsubdivisions=1\nwidth=%d\nheight=%d\nchannels=3\nmomentum=0.9\ndecay=0.0005\nlearning_rate=0.001\n"
            "burn_in=1000\nmax_batches=500200\npolicy=steps\nsteps=3000,5000\nscales=.1,.1\n\n" % (args.batch, args.size, args.size)
            + C.yolov3_single_cfg_text(1).replace("random=1", "random=0"))
    net = TrainableDarknet(text, device=dev, seed=1)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(0, 1, (args.batch, 3, args.size, args.size)).astype(np.float32)).to(dev)
    truth = np.zeros((args.batch, 90, 5), np.float32)
    truth[:, 0] = (.5, .5, .2, .3, 0)
    truth = torch.from_numpy(truth).to(dev)
    flops = {r: 0.0 for r in ROLES}
    for i, l in enumerate(net.convs):
        f = 2.0 * args.batch * l["out"][0] * l["out"][1] * l["out"][2] * l["cin"] * l["size"] ** 2
        flops[0] += f
        flops[1] += f
        flops[2] += f if i else 0.0
    spans, real_call, real_loss = [], net._call, net.loss

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def timed_call(name, *a):
        s = ev()
        real_call(name, *a)
        spans.append((ROLES[a[0]] if name == "bp_train_conv" else ("update" if "update" in name else "batch_norm"), s, ev()))

    def timed_loss(*a):
        s = ev()
        r = real_loss(*a)
        spans.append(("heads", s, ev()))
        return r
    real_update = net.update

    def timed_update():
        s = ev()
        real_update()
        spans.append(("update", s, ev()))
    net._call, net.loss, net.update = timed_call, timed_loss, timed_update
    rows = []
    for it in range(args.warmup + args.steps):
        del spans[:]
        s = ev()
        net.train_step(x, truth)
        e = ev()
        torch.cuda.synchronize()
        row = {"total": s.elapsed_time(e)}
        for k, a, b in spans:
            row[k] = row.get(k, 0.0) + a.elapsed_time(b)
        row["rest"] = row["total"] - sum(v for k, v in row.items() if k != "total")
        if it >= args.warmup:
            rows.append(row)
    out = {"net": "yolov3 single-class, %d x %d, batch %d" % (args.size, args.size, args.batch), "steps": args.steps, "ms": {}, "tflops": {}}
    for k in ("total", "forward", "filter_grad", "input_grad", "batch_norm", "update", "heads", "rest"):
        out["ms"][k] = stats([r.get(k, 0.0) for r in rows])
    for r, name in ROLES.items():
        out["tflops"][name] = flops[r] / (out["ms"][name]["median"] * 1e-3) / 1e12
    out["gflop_per_role"] = flops[0] / 1e9
    print(json.dumps(out), flush=True)          # (ours alone, before the comparison runs)
    deltas = [d.clone() for d in net.last_deltas]
    step = torch_iteration(torch, net, x, deltas)
    times = []
    for it in range(args.warmup + args.steps):
        s = ev()
        step()
        e = ev()
        torch.cuda.synchronize()
        if it >= args.warmup:
            times.append(s.elapsed_time(e))
    out["ms"]["torch_autograd"] = stats(times)
    print(json.dumps(out, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
