#!/usr/bin/env python3
"""What one training iteration of the key-point detector costs on the device: the reference's net
(FastPose_SE, 50 classes) at 320 x 256 through TrainableFastPose.train_step, timed with device events: the median of
``--steps`` iterations after ``--warmup``, with min and max; the time split by part (forward GEMMs, filter gradients,
input gradients, batch norm, tail / SE / pool, update, loss, the rest: zeroing, pixel shuffle and copies); the achieved
TFLOP/s of each GEMM role; the activation bytes one image holds; and the same iteration under torch autograd with
torch.optim.RMSprop on the same device.

    python tools/bench_kpd_train.py [--steps 10] [--warmup 2] [--batch 8] [--json profiles/kpd_train_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from betapose_amd.kpd_train import TrainableFastPose  # noqa: E402

PARTS = {"bp_kpd_train_bn_forward": "batch_norm", "bp_kpd_train_bn_backward": "batch_norm", "bp_kpd_train_tail_forward": "tail_se_pool",
         "bp_kpd_train_tail_backward": "tail_se_pool", "bp_kpd_train_pool_forward": "tail_se_pool", "bp_kpd_train_pool_backward": "tail_se_pool",
         "bp_kpd_train_sigmoid_forward": "tail_se_pool", "bp_kpd_train_sigmoid_backward": "tail_se_pool",
         "bp_kpd_train_maxpool_forward": "tail_se_pool", "bp_kpd_train_maxpool_backward": "tail_se_pool", "bp_kpd_train_rmsprop": "update"}
ROLES = {0: "forward_gemm", 1: "filter_grad", 2: "input_grad"}


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main(argv=None):
    import torch
    import kpd_train_common as K
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "kpd_train_bench.json"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    net = TrainableFastPose(device=dev, seed=0)
    rng = np.random.default_rng(0)
    B = a.batch
    inps = torch.from_numpy(rng.standard_normal((B, 3, 320, 256)).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rng.uniform(0, 1, (B, 50, 80, 64)).astype(np.float32)).to(dev)
    mask = torch.ones_like(labels)

    marks, flops = [], {r: 0.0 for r in ROLES.values()}
    real_call, real_loss = net._call, net._loss

    def timed(part, fn, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn(*args)
        e1.record()
        marks.append((part, e0, e1))
        return r

    def call(name, *args):
        part = PARTS.get(name)
        if part is None:
            part = ROLES[args[0]]
            N, C, H, W, Kc, size, stride = args[4:11]
            OH, OW = (H + 2 * (size // 2) - size) // stride + 1, (W + 2 * (size // 2) - size) // stride + 1
            flops[part] += 2.0 * N * OH * OW * Kc * C * size * size
        return timed(part, real_call, name, *args)

    net._call = call
    net._loss = lambda *args: timed("loss", real_loss, *args)
    totals, parts = [], {}
    for it in range(a.warmup + a.steps):
        marks.clear()
        for k in flops:
            flops[k] = 0.0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        net.train_step(inps, labels, mask)
        e1.record()
        torch.cuda.synchronize()
        if it < a.warmup:
            continue
        totals.append(e0.elapsed_time(e1))
        got = {}
        for part, s, e in marks:
            got[part] = got.get(part, 0.0) + s.elapsed_time(e)
        got["rest"] = totals[-1] - sum(got.values())
        for k, v in got.items():
            parts.setdefault(k, []).append(v)
    act = sum(b.numel() * b.element_size() for k, b in net._bufs.items() if k != "scratch")
    result = dict(device=torch.cuda.get_device_name(0), batch=B, input=[320, 256], steps=a.steps, warmup=a.warmup,
                  iteration_ms=stats(totals), parts_ms={k: stats(v) for k, v in sorted(parts.items())},
                  tflops={k: flops[k] / (float(np.median(parts[k])) * 1e-3) / 1e12 for k in flops},
                  gemm_flop_per_iteration=sum(flops.values()), activation_bytes_per_image=act // B,
                  scratch_bytes=int(net._bufs["scratch"].numel() * 4),
                  parameter_state_bytes=int(sum(p.numel() for k, p in net.P.items()) * 4 + sum(net.P[k].numel() for k in net.trainable) * 12))
    net._call, net._loss = real_call, real_loss
    del net._bufs
    # the same iteration under torch autograd
    P = {k: v.clone().requires_grad_(k in net.G) for k, v in net.P.items()}
    opt = torch.optim.RMSprop([P[k] for k in net.trainable], lr=1e-3)
    tt = []
    for it in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = K.mirror_forward(P, inps, net.stages, True)
        loss = torch.nn.functional.mse_loss(out * mask, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        e1.record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            tt.append(e0.elapsed_time(e1))
    result["torch_autograd_ms"] = stats(tt)
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
