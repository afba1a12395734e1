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

Bars.  Every recorded step is also evaluated in float64 by the numpy restatement of tests/darknet_train_f64.py
(``F64Net``: the formulas of DESIGN.md 3.13), fed the reference's recorded yolo deltas (group A) or, where calls follow
one another (groups B and C), yolo_loss(device=None) on its own heads.  Per quantity ``q`` the archive stores ``ref_err[q] = max|ref - f64| / max|f64|``; the tests' bar is ``max(4 * ref_err[q],
2^-23)`` and is read from the archive.

Conditions, enforced by re-seeding until the reference alone satisfies them, no case exempt: no convolution output
feeding a leaky activation within 1e-5 of zero; for the heads no best IoU within 1e-4 of ignore_thresh, no best / second
anchor IoU of a truth closer than 1e-6, no truth within 1e-4 of a cell edge; in group C the cost of call 20 is below
the cost of call 1.

The archive is written with fixed time stamps: running this twice gives the same bytes.

``python tools/make_golden_darknet_train.py shipped`` writes tests/golden/darknet_train_shipped.npz instead: one step of
the shipped topology on a 64 x 32 input (make_shipped).

Usage: python tools/make_golden_darknet_train.py [shipped]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_shims  # noqa: E402  (only for where the reference lies)
import darknet_train_common as D  # noqa: E402  (the seeded inputs and the quantity names the tests share)
from darknet_train_f64 import F64Net  # noqa: E402  (the one float64 text)
from betapose_amd import cfg as C  # noqa: E402
from betapose_amd.darknet_train import parse_layers  # noqa: E402  (the structure of the net only)
from betapose_amd.train_data import save_npz  # noqa: E402

SRC = os.path.join(ref_shims.REF, "train_YOLO", "src")
LIB = os.path.join(ROOT, "oracle", "_ref", "libdarknet_ref.so")
OUT = os.path.join(ROOT, "tests", "golden", "darknet_train.npz")
MAX_BOXES = 90
ANCHORS, tiny_cfg = D.ANCHORS, D.tiny_cfg
EPS_ZERO, EPS_IOU, EPS_ANCHOR, EPS_CELL = D.EPS_ZERO, D.EPS_IOU, D.EPS_ANCHOR, D.EPS_CELL
iou64, conditions = D.iou64, D.conditions
f32, f64 = np.float32, np.float64
NET_A = D.NET_A
NET_C = "learning_rate=0.002\npolicy=constant\nmax_batches=100\n"
POLICY_CFGS = {"constant": "policy=constant\n", "steps": "policy=steps\nsteps=6,9,12\nscales=.1,.5,2\n", "step": "policy=step\nstep=4\nscale=.3\n",
               "exp": "policy=exp\ngamma=.93\n", "poly": "policy=poly\npower=3\n"}
RATE_BATCHES = [0, 1, 2, 4, 5, 7, 10, 30]


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


def compile_driver(tmp):
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    driver = os.path.join(tmp, "darknet_train_ref_driver")
    subprocess.check_call(["gcc", "-O2", "-w", "-I", SRC, os.path.join(ROOT, "tools", "darknet_train_ref_driver.c"), "-o", driver,
                           "-L", os.path.dirname(LIB), "-ldarknet_ref", "-Wl,-rpath," + os.path.dirname(LIB), "-lm"])
    return driver


def make_shipped():
    """tests/golden/darknet_train_shipped.npz: one step of the shipped topology (D.shipped_cfg) by the reference.  Kept:
    the cfg, the seed, the checksum of the parameter bytes, the truth rows, the reference's yolo deltas, and per
    quantity ``ref_err``, the reference's distance from the float64 step fed its deltas and teacher-forced on ITS leaky
    masks -- at 1.4 M leaky outputs some pre-activations lie closer to 0 than float32 resolves, so the tiny nets'
    distance-to-zero condition cannot hold; instead the leaky outputs whose sign differs between the reference and the
    free float64 forward are counted, and a seed is refused where they exceed a quarter of the tests' cap.  No
    parameter and no activation is kept; the driver's 0.8 GB dump lives in the temporary directory."""
    text = D.shipped_cfg()
    net, layers, convs, heads = D.parsed(text)
    batch = net["batch"]
    with tempfile.TemporaryDirectory() as tmp:
        driver = compile_driver(tmp)
        seed = 900
        while True:
            st, x, truth = D.seeded_inputs(seed, text)
            recs, _ = run_reference(driver, tmp, text, convs, heads, st, [(x, truth)], 1, True, batch)
            r = recs[0]
            ok, gaps = conditions(r, convs, heads, truth, net, zero_gap=False)
            fed = [r["yolo%d.delta" % h] for h in range(len(heads))]
            masks = [r["fwd.conv%d.output" % n] > 0 if l["leaky"] else None for n, l in enumerate(convs)]
            exact, (flips, leaky) = D.f64_quantities(text, st, x, "shipped", fed, masks=masks)
            ok = ok and flips <= D.FLIP_CAP * leaky / 4
            if os.environ.get("DARKNET_TRAIN_GOLDEN_VERBOSE"):
                print("shipped", seed, ok, gaps, flips, leaky, float(r["cost"]), file=sys.stderr)
            if ok:
                break
            seed += 1
            if seed > 910:
                raise SystemExit("shipped: no seed satisfies the conditions")
    err = {q: rel_err(r[q[len("shipped.0."):]], v) for q, v in exact.items()}
    kept = max(int(np.flatnonzero(truth.any((0, 2))).max()) + 1, 1)
    arrays = {"truth": truth[:, :kept].copy()}
    for h, d in enumerate(fed):
        arrays["shipped.0.yolo%d.delta" % h] = d
    meta = dict(cfg=text, seed=seed, params_sha256=D.params_sha256(st), mask_flips=flips, leaky_outputs=leaky, flip_cap=D.FLIP_CAP,
                gaps=gaps, ref_err=err, restated=["F64Net (tests/darknet_train_f64.py), fed the reference's yolo deltas and its leaky masks"],
                reference_ran=["parse_network_cfg", "load_weights", "forward_network", "backward_network", "get_network_cost",
                               "update_network"])
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    out = os.path.join(ROOT, "tests", "golden", D.SHIPPED + ".npz")
    save_npz(out, arrays)
    print("wrote %s (%d bytes); %d of %d leaky outputs of the reference differ in sign from the free float64 run"
          % (out, os.path.getsize(out), flips, leaky))
    worst = {}
    for q, v in err.items():
        k = q.split(".")
        k = ".".join([k[2], k[-1]]) if len(k) > 3 else k[-1]
        worst[k] = max(worst.get(k, 0.0), v)
    print(json.dumps(worst, sort_keys=True, indent=1))


def main():
    arrays, err = {}, {}
    meta = {"reference_ran": ["parse_network_cfg", "load_weights", "train_network_datum", "forward_network", "backward_network",
                              "get_network_cost", "update_network", "get_current_rate", "save_weights"],
            "restated": ["F64Net: the step in float64 (numpy), fed the reference's yolo deltas or yolo_loss(device=None)"],
            "conditions": {"leaky_input_to_zero": EPS_ZERO, "iou_to_threshold": EPS_IOU, "anchor_gap": EPS_ANCHOR, "cell_to_integer": EPS_CELL,
                           "group_c_cost_falls": 1}, "exempt_cases": 0, "max_boxes": MAX_BOXES, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        driver = compile_driver(tmp)
        # name, width, height, net batch, subdivisions, classes, [net] extras, calls, one fixed batch, detail
        for name, width, height, batch, sub, classes, extra, calls, fixed, detail in (
                ("a0", 16, 16, 3, 1, 1, NET_A, 1, True, True), ("a1", 24, 16, 1, 1, 3, NET_A, 1, True, True),
                ("b", 16, 16, 2, 2, 1, NET_A, 4, False, True), ("c", 16, 16, 3, 1, 1, NET_C, 20, True, False)):
            text, net, layers, convs, heads = build(width, height, batch, sub, classes, extra)
            seed = 900
            while True:
                rng = np.random.default_rng([seed, width, batch, classes, calls])
                st = D.seeded_state(rng, convs, classes)
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
    make_shipped() if sys.argv[1:] == ["shipped"] else main()
