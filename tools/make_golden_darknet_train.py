#!/usr/bin/env python3
"""Generate tests/golden/darknet_train.npz by running the REFERENCE's own Darknet C code (build machine only; nothing of
the reference is copied).  The project's own driver tools/darknet_train_ref_driver.c is compiled against the
reference's headers and ``oracle/_ref/libdarknet_ref.so`` (oracle/Makefile) into a temporary directory; the tiny cfgs
are written here and hold settings only.

  group A  one step (subdivisions = 1) of the tiny two-head net of ``tiny_cfg`` at 16 x 16, batch 3, classes 1 and at
           24 x 16, batch 1, classes 3.  Recorded: inputs, truth, initial parameters; from the reference every
           convolution's output, batch mean and variance, every weight / bias / scale update buffer before the update,
           every parameter, rolling statistic and update buffer after it, the cost and the two yolo layers' deltas.
  group B  the same net with batch=4 subdivisions=2, four calls (two updates, the second with momentum carried), the
           state after each call; get_current_rate at 8 batch numbers across burn_in for each of the five policies.
  group C  20 calls on one fixed batch: the cost sequence, the final parameters, the bytes of save_weights' file.

Bars.  Every recorded step is also evaluated in float64 by the numpy restatement below (``F64Net``: the formulas of
DESIGN.md 3.13), fed the reference's recorded yolo deltas (group A) or, where calls follow one another (groups B and C),
yolo_loss(device=None) on its own heads.  Per
quantity ``q`` the archive stores ``ref_err[q] = max|ref - f64| / max|f64|``; the tests' bar is ``max(4 * ref_err[q],
2^-23)`` and is read from the archive.

Conditions, enforced by re-seeding until the reference alone satisfies them, no case exempt: no convolution output
feeding a leaky activation within 1e-5 of zero; for the heads no best IoU within 1e-4 of ignore_thresh, no best / second
anchor IoU of a truth closer than 1e-6, no truth within 1e-4 of a cell edge; in group C the cost of call 20 is below
the cost of call 1.

The archive is written with fixed time stamps: running this twice gives the same bytes.

Usage: python tools/make_golden_darknet_train.py
"""
from __future__ import annotations

import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_shims  # noqa: E402  (only for where the reference lies)
from betapose_amd import cfg as C  # noqa: E402
from betapose_amd.darknet_train import learning_rate, parse_layers  # noqa: E402  (the structure of the net only)
from betapose_amd.train_data import save_npz  # noqa: E402
from betapose_amd.yolo_train import yolo_loss  # noqa: E402

SRC = os.path.join(ref_shims.REF, "train_YOLO", "src")
LIB = os.path.join(ROOT, "oracle", "_ref", "libdarknet_ref.so")
OUT = os.path.join(ROOT, "tests", "golden", "darknet_train.npz")
MAX_BOXES = 90
ANCHORS = [(2, 3), (4, 3), (3, 5), (6, 8), (10, 7), (12, 13)]
EPS_ZERO, EPS_IOU, EPS_ANCHOR, EPS_CELL = 1e-5, 1e-4, 1e-6, 1e-4
f32, f64 = np.float32, np.float64
NET_A = "learning_rate=0.01\nburn_in=3\npolicy=steps\nsteps=2,10\nscales=.5,.1\nmax_batches=100\n"
NET_C = "learning_rate=0.002\npolicy=constant\nmax_batches=100\n"
POLICY_CFGS = {"constant": "policy=constant\n", "steps": "policy=steps\nsteps=6,9,12\nscales=.1,.5,2\n", "step": "policy=step\nstep=4\nscale=.3\n",
               "exp": "policy=exp\ngamma=.93\n", "poly": "policy=poly\npower=3\n"}
RATE_BATCHES = [0, 1, 2, 4, 5, 7, 10, 30]


def tiny_cfg(width, height, batch, subdivisions, classes, net_extra):
    A = 3 * (5 + classes)

    def conv(filters, size, stride, bn=True, act="leaky"):
        return ("[convolutional]\n" + ("batch_normalize=1\n" if bn else "") +
                "filters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n" % (filters, size, stride, act))

    def yolo(mask):
        return ("[yolo]\nmask = %s\nanchors = %s\nclasses=%d\nnum=%d\njitter=.3\nignore_thresh = .7\ntruth_thresh = 1\nrandom=0\n\n"
                % (",".join(str(m) for m in mask), ",  ".join("%d,%d" % a for a in ANCHORS), classes, len(ANCHORS)))
    return ("[net]\nbatch=%d\nsubdivisions=%d\nwidth=%d\nheight=%d\nchannels=3\nmomentum=0.9\ndecay=0.0005\n%s\n"
            % (batch, subdivisions, width, height, net_extra) +
            conv(6, 3, 1) + conv(10, 3, 2) + conv(5, 1, 1) + conv(10, 3, 1) + "[shortcut]\nfrom=-3\nactivation=linear\n\n" +
            conv(12, 3, 2) + conv(A, 1, 1, False, "linear") + yolo((3, 4, 5)) + "[route]\nlayers = -4\n\n" + conv(6, 1, 1) +
            "[upsample]\nstride=2\n\n" + "[route]\nlayers = -1, 0\n\n" + conv(8, 3, 1) + conv(A, 1, 1, False, "linear") + yolo((0, 1, 2)))


def initial_state(rng, convs, classes):
    st = {}
    for n, l in enumerate(convs):
        K, c, s = l["out"][0], l["cin"], l["size"]
        p = "conv%d." % n
        if l["bn"]:
            st[p + "weights"] = rng.normal(0, 1.0 / np.sqrt(c * s * s), (K, c, s, s)).astype(f32)
            st[p + "biases"] = rng.normal(0, .2, K).astype(f32)
            st[p + "scales"] = rng.uniform(.8, 1.2, K).astype(f32)
            st[p + "rolling_mean"] = rng.normal(0, .3, K).astype(f32)
            st[p + "rolling_variance"] = rng.uniform(.5, 1.5, K).astype(f32)
        else:       # a head: modest box terms, objectness biased low
            scale = np.tile(np.array([.5, .5, .15, .15, .6] + [.4] * classes, f32), 3)
            st[p + "weights"] = (rng.normal(0, 1, (K, c, 1, 1)).astype(f32) * scale[:, None, None, None]).astype(f32)
            st[p + "biases"] = np.tile(np.array([0, 0, 0, 0, -2.0] + [0.0] * classes, f32), 3)
    return st


def weights_bytes(convs, st, seen=0):
    w = struct.pack("<iiii", 0, 1, 0, seen)
    for n, l in enumerate(convs):
        for k in ("biases", "scales", "rolling_mean", "rolling_variance", "weights"):
            if "conv%d.%s" % (n, k) in st:
                w += np.ascontiguousarray(st["conv%d.%s" % (n, k)], f32).tobytes()
    return w


def make_truth(rng, batch, classes, width, height):
    """rows (x, y, w, h, id) sized about the anchors; one image with two boxes, the last image of a batch > 1 with none"""
    t = np.zeros((batch, MAX_BOXES, 5), f32)
    for b in range(batch):
        if batch > 1 and b == batch - 1:
            continue
        for k in range(2 if b == 0 else 1):
            a = np.array(ANCHORS[rng.integers(0, len(ANCHORS))], f64) * rng.uniform(.8, 1.2, 2)
            t[b, k] = (rng.uniform(.15, .85), rng.uniform(.15, .85), a[0] / width, a[1] / height, rng.integers(0, classes))
    return t


# ------------------------------------------------------------------------------------------------ the float64 restatement
class F64Net:
    """forward with batch statistics, backward and update of DESIGN.md 3.13 in float64"""

    def __init__(self, net, layers, st):
        self.net, self.layers = net, layers
        self.convs = [l for l in layers if l["type"] == "convolutional"]
        self.st = {k: v.astype(f64) for k, v in st.items()}
        for n, l in enumerate(self.convs):
            for k, src in (("weight_updates", "weights"), ("bias_updates", "biases"), ("scale_updates", "scales")):
                if "conv%d.%s" % (n, src) in self.st:
                    self.st.setdefault("conv%d.%s" % (n, k), np.zeros_like(self.st["conv%d.%s" % (n, src)]))
        self.seen = 0

    @staticmethod
    def cols(x, s, stride):
        p = s // 2
        N, c, H, W = x.shape
        OH, OW = (H + 2 * p - s) // stride + 1, (W + 2 * p - s) // stride + 1
        xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
        return np.stack([xp[:, :, ky:ky + stride * OH:stride, kx:kx + stride * OW:stride] for ky in range(s) for kx in range(s)], 2)

    def forward(self, x):
        x = x.astype(f64)
        self.inp, outs, heads, rec, n = x, [], [], {}, 0
        for l in self.layers:
            t = l["type"]
            if t == "convolutional":
                p = "conv%d." % n
                w = self.st[p + "weights"]
                K, c, s = w.shape[:3]
                l["cols"] = self.cols(x, s, l["stride"])
                raw = np.einsum("nctyx,kct->nkyx", l["cols"], w.reshape(K, c, s * s))
                if l["bn"]:
                    cnt = raw.shape[0] * raw.shape[2] * raw.shape[3]
                    mean = raw.mean((0, 2, 3))
                    var = ((raw - mean[None, :, None, None]) ** 2).sum((0, 2, 3)) / (cnt - 1)
                    for k, v in (("rolling_mean", mean), ("rolling_variance", var)):
                        self.st[p + k] = .9 * self.st[p + k] + .1 * v
                    xn = (raw - mean[None, :, None, None]) / (np.sqrt(var) + 1e-6)[None, :, None, None]
                    l.update(x=raw, x_norm=xn, mean=mean, var=var)
                    rec[p + "mean"], rec[p + "variance"] = mean, var
                    raw = xn * self.st[p + "scales"][None, :, None, None]
                raw = raw + self.st[p + "biases"][None, :, None, None]
                x = np.where(raw > 0, raw, .1 * raw) if l["leaky"] else raw
                rec[p + "output"] = x
                n += 1
            elif t == "shortcut":
                x = x + outs[l["src"]]
            elif t == "route":
                x = np.concatenate([outs[s] for s in l["src"]], 1)
            elif t == "upsample":
                x = x.repeat(2, 2).repeat(2, 3)
            else:
                heads.append(x)
            outs.append(x)
        self.outs = outs
        return heads, rec

    def backward(self, head_deltas):
        deltas = [np.zeros_like(o) for o in self.outs]
        hd, n = list(head_deltas), len(self.convs)
        for i in range(len(self.layers) - 1, -1, -1):
            l, t, d = self.layers[i], self.layers[i]["type"], deltas[i]
            if t == "yolo":
                deltas[i - 1] += hd.pop().astype(f64)
            elif t == "convolutional":
                n -= 1
                p = "conv%d." % n
                out = self.outs[i]
                d = d * np.where(out > 0, 1.0, .1) if l["leaky"] else d
                self.st[p + "bias_updates"] += d.sum((0, 2, 3))
                if l["bn"]:
                    cnt = d.shape[0] * d.shape[2] * d.shape[3]
                    mean, var = l["mean"][None, :, None, None], l["var"][None, :, None, None]
                    self.st[p + "scale_updates"] += (d * l["x_norm"]).sum((0, 2, 3))
                    d = d * self.st[p + "scales"][None, :, None, None]
                    md = d.sum((0, 2, 3), keepdims=True) * (-1. / np.sqrt(var + 1e-5))
                    vd = (d * (l["x"] - mean)).sum((0, 2, 3), keepdims=True) * -.5 * (var + 1e-5) ** -1.5
                    d = d / (np.sqrt(var) + 1e-5) + vd * 2. * (l["x"] - mean) / cnt + md / cnt
                w = self.st[p + "weights"]
                K, c, s = w.shape[:3]
                self.st[p + "weight_updates"] += np.einsum("nkyx,nctyx->kct", d, l["cols"]).reshape(w.shape)
                if i:
                    dc = np.einsum("nkyx,kct->nctyx", d, w.reshape(K, c, s * s))
                    pd, st = s // 2, l["stride"]
                    N, _, H, W = deltas[i - 1].shape
                    OH, OW = d.shape[2:]
                    buf = np.zeros((N, c, H + 2 * pd, W + 2 * pd))
                    for ky in range(s):
                        for kx in range(s):
                            buf[:, :, ky:ky + st * OH:st, kx:kx + st * OW:st] += dc[:, :, ky * s + kx]
                    deltas[i - 1] += buf[:, :, pd:pd + H, pd:pd + W]
            elif t == "shortcut":
                deltas[i - 1] += d
                deltas[l["src"]] += d
            elif t == "route":
                at = 0
                for s_ in l["src"]:
                    c = self.outs[s_].shape[1]
                    deltas[s_] += d[:, at:at + c]
                    at += c
            elif t == "upsample":
                deltas[i - 1] += d[:, :, 0::2, 0::2] + d[:, :, 0::2, 1::2] + d[:, :, 1::2, 0::2] + d[:, :, 1::2, 1::2]

    def update(self):
        ub = self.net["batch"] * self.net["subdivisions"]
        rate = float(learning_rate(self.net, self.seen // ub))
        mom, decay = float(self.net["momentum"]), float(self.net["decay"])
        for n, l in enumerate(self.convs):
            p = "conv%d." % n
            for k, u in (("biases", "bias_updates"), ("scales", "scale_updates"), ("weights", "weight_updates")):
                if p + k not in self.st:
                    continue
                if k == "weights":
                    self.st[p + u] = self.st[p + u] - decay * ub * self.st[p + k]
                self.st[p + k] = self.st[p + k] + rate / ub * self.st[p + u]
                self.st[p + u] = self.st[p + u] * mom

    def step(self, x, head_deltas=None, truth=None):
        """one train_network_datum: (cost, the forward's record, the update buffers before the update)"""
        self.seen += self.net["batch"]
        heads, rec = self.forward(x)
        costs = None
        if head_deltas is None:
            head_deltas, costs = [], []
            for l, h in zip([l for l in self.layers if l["type"] == "yolo"], heads):
                p = l["head"]
                c, _, d, _ = yolo_loss(h.astype(f32), truth, (self.net["height"], self.net["width"]), p["anchors"], p["mask"], p["classes"],
                                       p["ignore_thresh"], p["truth_thresh"], want_act=False)
                head_deltas.append(d), costs.append(c)
        self.backward(head_deltas)
        pre = {k: v.copy() for k, v in self.st.items() if k.endswith("_updates")}
        if (self.seen // self.net["batch"]) % self.net["subdivisions"] == 0:
            self.update()
        return (None if costs is None else float(np.mean(costs))), rec, pre


# ------------------------------------------------------------------------------------------------ the reference
def sizes(convs, batch):
    """per convolution (elements of its output, K, elements of its filters)"""
    return [(batch * l["out"][0] * l["out"][1] * l["out"][2], l["out"][0], l["out"][0] * l["cin"] * l["size"] ** 2) for l in convs]


def run_reference(driver, tmp, cfg_text, convs, heads, st, batches, calls, detail, batch):
    """the dump of the driver as a list per call of dicts of float32 arrays, and the bytes of its save_weights file"""
    paths = {k: os.path.join(tmp, k) for k in ("net.cfg", "in.weights", "batches.bin", "dump.bin", "out.weights")}
    open(paths["net.cfg"], "w").write(cfg_text)
    open(paths["in.weights"], "wb").write(weights_bytes(convs, st))
    with open(paths["batches.bin"], "wb") as f:
        for x, t in batches:
            f.write(np.ascontiguousarray(x, f32).tobytes() + np.ascontiguousarray(t, f32).tobytes())
    subprocess.run([driver, "train", paths["net.cfg"], paths["in.weights"], paths["batches.bin"], str(calls), str(int(detail)),
                    paths["dump.bin"], paths["out.weights"]], check=True, cwd=tmp, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    raw = np.fromfile(paths["dump.bin"], f32)
    at, out = 0, []

    def take(n, shape=None):
        nonlocal at
        v = raw[at:at + n].copy()
        at += n
        return v if shape is None else v.reshape(shape)
    for _ in range(calls):
        r = {"cost": take(1)[0], "rate": take(1)[0]}
        if detail:
            hi = 0
            for n, l in enumerate(convs):
                p = "conv%d." % n
                no, K, nw = sizes(convs, batch)[n]
                shape = (batch,) + l["out"]
                r["fwd." + p + "output"] = take(no, shape)
                if l["bn"]:
                    r["fwd." + p + "x"], r["fwd." + p + "mean"], r["fwd." + p + "variance"] = take(no, shape), take(K), take(K)
                r["pre." + p + "weight_updates"], r["pre." + p + "bias_updates"] = take(nw, (K, l["cin"], l["size"], l["size"])), take(K)
                if l["bn"]:
                    r["pre." + p + "scale_updates"] = take(K)
                if l.get("is_head"):
                    h = heads[hi]
                    r["yolo%d.delta" % hi] = take(batch * h["out"][0] * h["out"][1] * h["out"][2], (batch,) + h["out"])
                    hi += 1
        for n, l in enumerate(convs):
            p = "post.conv%d." % n
            K, nw, ws = l["out"][0], sizes(convs, batch)[n][2], (l["out"][0], l["cin"], l["size"], l["size"])
            r[p + "biases"] = take(K)
            if l["bn"]:
                r[p + "scales"], r[p + "rolling_mean"], r[p + "rolling_variance"] = take(K), take(K), take(K)
            r[p + "weights"], r[p + "bias_updates"] = take(nw, ws), take(K)
            if l["bn"]:
                r[p + "scale_updates"] = take(K)
            r[p + "weight_updates"] = take(nw, ws)
        out.append(r)
    assert at == len(raw), (at, len(raw))
    return out, open(paths["out.weights"], "rb").read()


def iou64(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)

    def ov(x1, w1, x2, w2):
        return np.minimum(x1 + w1 / 2, x2 + w2 / 2) - np.maximum(x1 - w1 / 2, x2 - w2 / 2)
    w, h = ov(a[..., 0], a[..., 2], b[..., 0], b[..., 2]), ov(a[..., 1], a[..., 3], b[..., 1], b[..., 3])
    inter = np.where((w < 0) | (h < 0), 0.0, w * h)
    return inter / (a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter)


def conditions(rec, convs, heads, truth, net):
    """whether one detailed call of the reference stays inside the conditions, and the margins"""
    zero = 1.0
    for n, l in enumerate(convs):
        if l["leaky"]:
            o = rec["fwd.conv%d.output" % n].astype(f64)
            pre = np.where(o > 0, o, o / .1)
            zero = min(zero, float(np.abs(pre).min()))
    gi = ga = gc = 1.0
    nw, nh = net["width"], net["height"]
    anc = np.array(ANCHORS, f64)
    anchors = np.stack([np.zeros(len(anc)), np.zeros(len(anc)), anc[:, 0] / nw, anc[:, 1] / nh], -1)
    hi = 0
    for n, l in enumerate(convs):
        if not l.get("is_head"):
            continue
        p = heads[hi]["head"]
        hi += 1
        x = rec["fwd.conv%d.output" % n].astype(f64)
        B, _, h, w = x.shape
        a = x.reshape(B, len(p["mask"]), 5 + p["classes"], h, w)
        jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        sg = lambda v: 1. / (1. + np.exp(-v))
        aw, ah = anc[p["mask"], 0][None, :, None, None], anc[p["mask"], 1][None, :, None, None]
        pred = np.stack([(ii + sg(a[:, :, 0])) / w, (jj + sg(a[:, :, 1])) / h, np.exp(a[:, :, 2]) * aw / nw, np.exp(a[:, :, 3]) * ah / nh], -1)
        for b in range(B):
            rows = np.array([t for t in truth[b] if t[0] != 0], f64).reshape(-1, 5)
            if not len(rows):
                continue
            best = iou64(pred[b][..., None, :], rows[:, :4]).max(-1)
            gi = min(gi, float(np.abs(best - p["ignore_thresh"]).min()))
            for t in rows:
                s = np.sort(iou64(anchors, np.array([0, 0, t[2], t[3]])))
                ga = min(ga, float(s[-1] - s[-2]))
                fx, fy = t[0] * w, t[1] * h
                gc = min(gc, abs(fx - round(fx)), abs(fy - round(fy)))
    return zero > EPS_ZERO and gi > EPS_IOU and ga > EPS_ANCHOR and gc > EPS_CELL, dict(zero=zero, iou=gi, anchor=ga, cell=gc)


def rel_err(ref, exact):
    ref, exact = np.asarray(ref, f64), np.asarray(exact, f64)
    m = float(np.abs(exact).max())
    return float(np.abs(ref - exact).max() / m) if m > 0 else 0.0


def build(width, height, batch, subdivisions, classes, net_extra):
    text = tiny_cfg(width, height, batch * subdivisions, subdivisions, classes, net_extra)
    net, layers = parse_layers(C.parse_cfg_text(text))
    convs = [l for l in layers if l["type"] == "convolutional"]
    for i, l in enumerate(layers):
        if l["type"] == "yolo":
            layers[i - 1]["is_head"] = True
    return text, net, layers, convs, [l for l in layers if l["type"] == "yolo"]


def main():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    arrays, err = {}, {}
    meta = {"reference_ran": ["parse_network_cfg", "load_weights", "train_network_datum", "forward_network", "backward_network",
                              "get_network_cost", "update_network", "get_current_rate", "save_weights"],
            "restated": ["F64Net: the step in float64 (numpy), fed the reference's yolo deltas or yolo_loss(device=None)"],
            "conditions": {"leaky_input_to_zero": EPS_ZERO, "iou_to_threshold": EPS_IOU, "anchor_gap": EPS_ANCHOR, "cell_to_integer": EPS_CELL,
                           "group_c_cost_falls": 1}, "exempt_cases": 0, "max_boxes": MAX_BOXES, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        driver = os.path.join(tmp, "darknet_train_ref_driver")
        subprocess.check_call(["gcc", "-O2", "-w", "-I", SRC, os.path.join(ROOT, "tools", "darknet_train_ref_driver.c"), "-o", driver,
                               "-L", os.path.dirname(LIB), "-ldarknet_ref", "-Wl,-rpath," + os.path.dirname(LIB), "-lm"])
        # name, width, height, net batch, subdivisions, classes, [net] extras, calls, one fixed batch, detail
        for name, width, height, batch, sub, classes, extra, calls, fixed, detail in (
                ("a0", 16, 16, 3, 1, 1, NET_A, 1, True, True), ("a1", 24, 16, 1, 1, 3, NET_A, 1, True, True),
                ("b", 16, 16, 2, 2, 1, NET_A, 4, False, True), ("c", 16, 16, 3, 1, 1, NET_C, 20, True, False)):
            text, net, layers, convs, heads = build(width, height, batch, sub, classes, extra)
            seed = 900
            while True:
                rng = np.random.default_rng([seed, width, batch, classes, calls])
                st = initial_state(rng, convs, classes)
                batches = [(rng.uniform(0, 1, (batch, 3, height, width)).astype(f32), make_truth(rng, batch, classes, width, height))
                           for _ in range(1 if fixed else calls)]
                recs, wfile = run_reference(driver, tmp, text, convs, heads, st, batches, calls, detail, batch)
                ok, gaps = True, {}
                if detail:
                    for k, r in enumerate(recs):
                        good, g = conditions(r, convs, heads, batches[0 if fixed else k][1], net)
                        ok = ok and good
                        gaps = {q: min(v, gaps.get(q, 1.0)) for q, v in g.items()}
                else:       # the conditions on a run without detail are tested on a detailed rerun of its first call
                    r1, _ = run_reference(driver, tmp, text, convs, heads, st, batches, 1, True, batch)
                    ok, gaps = conditions(r1[0], convs, heads, batches[0][1], net)
                    ok = ok and recs[-1]["cost"] < recs[0]["cost"]
                if os.environ.get("DARKNET_TRAIN_GOLDEN_VERBOSE"):
                    print(name, seed, ok, gaps, [float(r["cost"]) for r in recs], file=sys.stderr)
                if ok:
                    break
                seed += 1
                if seed > 960:
                    raise SystemExit("%s: no seed satisfies the conditions" % name)
            # the float64 evaluation of the same calls
            ex, exact_costs = F64Net(net, layers, st), []
            for k, r in enumerate(recs):
                x, t = batches[0 if fixed else k]
                fed = detail and name != "b"        # group B runs on, as group C does, so its float64 evaluation forms its own deltas
                cost, rec, pre = ex.step(x, [r["yolo%d.delta" % h] for h in range(len(heads))] if fed else None, t)
                if detail:
                    err["%s.%d.cost" % (name, k)] = rel_err(r["cost"], cost if not fed else np.mean(
                        [(r["yolo%d.delta" % h].astype(f64) ** 2).sum() for h in range(len(heads))]))
                    for q, v in rec.items() if name != "b" else ():
                        err["%s.%d.fwd.%s" % (name, k, q)] = rel_err(r["fwd." + q], v)
                    for q, v in pre.items() if name != "b" else ():
                        err["%s.%d.pre.%s" % (name, k, q)] = rel_err(r["pre." + q], v)
                    for q, v in ex.st.items():
                        err["%s.%d.post.%s" % (name, k, q)] = rel_err(r["post." + q], v)
                else:
                    exact_costs.append(cost)
                    if k == calls - 1:
                        for q, v in ex.st.items():
                            err["%s.%d.post.%s" % (name, k, q)] = rel_err(r["post." + q], v)
            for q, v in st.items():
                arrays["%s.init.%s" % (name, q)] = v
            for k, (x, t) in enumerate(batches):
                arrays["%s.%d.inps" % (name, k)], arrays["%s.%d.truth" % (name, k)] = x, t[:, :4].copy()
            for k, r in enumerate(recs):
                for q, v in r.items():
                    # group B keeps the state after each call (its forward record only feeds the float64 evaluation here)
                    keep = (q in ("cost", "rate") or (q.startswith("post.") and (name == "b" or k == calls - 1)) or
                            (detail and name != "b"))
                    if keep and not q.endswith(".x"):
                        arrays["%s.%d.%s" % (name, k, q)] = np.asarray(v, f32)
            if name == "c":     # the cost sequence is one quantity: a vector of `calls` values
                arrays["c.costs"] = np.array([r["cost"] for r in recs], f32)
                err["c.costs"] = rel_err(arrays["c.costs"], exact_costs)
                arrays["c.weights_file"] = np.frombuffer(wfile, np.uint8)
            meta["cases"][name] = dict(cfg=text, width=width, height=height, batch=batch, subdivisions=sub, classes=classes, calls=calls,
                                       fixed_batch=fixed, detail=detail, seed=seed, gaps=gaps, truth_rows_kept=4)
        # the schedule
        meta["rates"] = {}
        for pol, extra in POLICY_CFGS.items():
            text = tiny_cfg(16, 16, 4, 2, 1, "learning_rate=0.013\nburn_in=5\nmax_batches=40\n" + extra)
            p = os.path.join(tmp, "rate_%s.cfg" % pol)
            open(p, "w").write(text)
            subprocess.run([driver, "rates", p, os.path.join(tmp, "rates.bin")] + [str(b) for b in RATE_BATCHES], check=True, cwd=tmp,
                           stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            arrays["rates." + pol] = np.fromfile(os.path.join(tmp, "rates.bin"), f32)
            meta["rates"][pol] = dict(cfg=text, batches=RATE_BATCHES)
    meta["ref_err"] = err
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    save_npz(OUT, arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    worst = {}
    for q, v in err.items():
        k = q.split(".")        # <case>.<call>.<stage>.conv<n>.<name>, <case>.<call>.cost or c.costs
        k = ".".join([k[2], k[-1]]) if len(k) > 3 else k[-1]
        worst[k] = max(worst.get(k, 0.0), v)
    print(json.dumps(worst, sort_keys=True, indent=1))


if __name__ == "__main__":
    main()
