#!/usr/bin/env python3
"""Generate tests/golden/yolo_map.npz by running the REFERENCE's own Darknet C code (build machine only; nothing of the
reference is copied).  The project's own driver tools/yolo_map_ref_driver.c is compiled against the reference's headers
and ``oracle/_ref/libdarknet_ref.so`` (oracle/Makefile) into a temporary directory.

  group A  the box list.  Yolo heads filled here (activated values, Darknet's layout) go through ``get_network_boxes(net,
           1, 1, thresh, 0, 0, 0, &n, 0)`` and ``do_nms_sort``: heads 2 x 2 + 4 x 4 (60 rows), 13 x 13 alone (507), 13 x 13 + 26 x 26 (2 535
           rows) and one 3 x 2 head, classes 1 and 3, images with 0, 1, about 100 and more than 1 024 candidates, one
           ``nms = 0`` case.  A second run with nms = 0 gives the candidates in Darknet's order, from which every
           survivor's candidate index is looked up.  Recorded: the head values as 16-bit steps (the tests form ``pred`` from them with
           the same float32 decode, tests/yolo_map_common.py), the candidate index of every entry in the order
           do_nms_sort left, and the rows (box, objectness, probs) of the entries that keep a non-zero prob.
  group B  the accounting.  ``validate_detector_map`` itself on a tiny cfg (written here, settings only), random
           weights and 12 small PNG frames each with label files at 64 x 64 (the smallest input the detector engine takes): classes 1 (one 4 x 4 head) and 3 (heads 4 x 4 and 2 x 2).
           The labels are placed from the reference's own detections so that true positives, duplicate detections of
           one truth, a frame without a label, a black frame without a detection and a class with exactly 10 truths
           (three or more of them found) all occur.  Recorded: the report's numbers, and per frame the heads' l.output
           as ``pred``, so the accounting can be fed the reference's own predictions.

Conditions, enforced by re-seeding until the reference alone stays inside them, with no exempt case: no box_iou (numpy
float64 of the reference's boxes) within 1e-4 of nms among an image's candidates or of iou_thresh between a detection
and a label; no prob within 1e-6 of thresh or thresh_calc; no two equal non-zero probs within a group A image or within a
group B run; no two labels whose IoUs with one detection tie.

The archive is written with fixed time stamps: running this twice gives the same bytes.

Usage: python tools/make_golden_yolo_map.py
"""
from __future__ import annotations

import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_shims  # noqa: E402  (only for where the reference lies)
from betapose_amd.train_data import save_npz  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yolo_map_common import ANCHORS as ANCH_A, decode_pred, heads_from_u16  # noqa: E402  (the tests decode the same way)

SRC = os.path.join(ref_shims.REF, "train_YOLO", "src")
LIB = os.path.join(ROOT, "oracle", "_ref", "libdarknet_ref.so")
OUT = os.path.join(ROOT, "tests", "golden", "yolo_map.npz")
THRESH, NMS, IOU_THRESH, THRESH_CALC = 0.005, 0.45, 0.5, 0.25
EPS_IOU, EPS_PROB = 1e-4, 1e-6
f32 = np.float32


def iou64(a, b):
    """box_iou in float64, broadcasting over [..., 4] = (x, y, w, h)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)

    def ov(x1, w1, x2, w2):
        return np.minimum(x1 + w1 / 2, x2 + w2 / 2) - np.maximum(x1 - w1 / 2, x2 - w2 / 2)
    w, h = ov(a[..., 0], a[..., 2], b[..., 0], b[..., 2]), ov(a[..., 1], a[..., 3], b[..., 1], b[..., 3])
    inter = np.where((w < 0) | (h < 0), 0.0, w * h)
    return inter / (a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter)


def run_boxes(driver, tmp, outs, heads, anchors, net_w, net_h, classes, thresh, nms):
    inp, out = os.path.join(tmp, "boxes.in"), os.path.join(tmp, "boxes.out")
    with open(inp, "wb") as f:
        f.write(np.array([len(heads), classes, len(anchors), net_w, net_h], np.int32).tobytes())
        f.write(np.array([thresh, nms], f32).tobytes())
        f.write(np.ascontiguousarray(anchors, f32).tobytes())
        for o, (n, gh, gw, mask) in zip(outs, heads):
            f.write(np.array([n, gh, gw] + list(mask), np.int32).tobytes())
            f.write(np.ascontiguousarray(o, f32).tobytes())
    subprocess.run([driver, "boxes", inp, out], check=True, cwd=tmp, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL)
    raw = open(out, "rb").read()
    n = struct.unpack("i", raw[:4])[0]
    return np.frombuffer(raw[4:], f32).reshape(n, 5 + classes).copy()


def survivors(driver, tmp, outs, heads, anchors, net_w, net_h, classes, nms):
    """(rows [n, 5 + classes] after do_nms_sort, candidate index of each, candidates in Darknet's order)"""
    cand = run_boxes(driver, tmp, outs, heads, anchors, net_w, net_h, classes, THRESH, 0.0)
    dets = run_boxes(driver, tmp, outs, heads, anchors, net_w, net_h, classes, THRESH, nms) if nms else cand.copy()
    where = {}
    for i, r in enumerate(cand):
        where.setdefault(r[:5].tobytes(), []).append(i)
    idx = np.array([where[r[:5].tobytes()].pop(0) for r in dets], np.int32) if len(dets) else np.zeros(0, np.int32)
    return dets, idx, cand


def list_gaps(cand, nms):
    """the margins of one image's candidates: (IoU to nms, prob to thresh, whether two non-zero probs are equal)"""
    gi = 1.0
    if nms and len(cand) > 1:
        for s in range(0, len(cand), 256):
            m = iou64(cand[s:s + 256, None, :4], cand[None, :, :4])
            gi = min(gi, float(np.nanmin(np.abs(m - nms))))
    p = cand[:, 5:].astype(np.float64)
    gp = float(np.abs(p[p > 0] - THRESH).min()) if (p > 0).any() else 1.0
    gp = min(gp, float(np.abs(cand[:, 4].astype(np.float64) - THRESH).min()) if len(cand) else 1.0)
    equal = any(len(np.unique(p[:, k][p[:, k] > 0])) != (p[:, k] > 0).sum() for k in range(p.shape[1]))
    return gi, gp, equal


# ---------------------------------------------------------------------------------------------------- group A
SMALL = [(3, 2, 2, (3, 4, 5)), (3, 4, 4, (0, 1, 2))]
BIG = [(3, 13, 13, (3, 4, 5)), (3, 26, 26, (0, 1, 2))]
MID = [(3, 13, 13, (3, 4, 5))]
WIDE = [(3, 2, 3, (0, 1, 2))]
# name, heads, (net_w, net_h), classes, nms, fraction of rows above thresh (None: exactly one)
CASES_A = [("empty_c1", SMALL, (64, 64), 1, NMS, 0.0), ("one_c1", SMALL, (64, 64), 1, NMS, None), ("small_c3", SMALL, (64, 64), 3, NMS, 1.0),
           ("small_c3_nms0", SMALL, (64, 64), 3, 0.0, 0.8), ("wide_c3", WIDE, (96, 64), 3, NMS, 1.0),
           ("mid100_c1", MID, (416, 416), 1, NMS, 0.2), ("big_all_c1", BIG, (416, 416), 1, NMS, 1.0),
           ("mid_c3", MID, (416, 416), 3, NMS, 0.6)]


def make_heads(rng, heads, classes, frac):
    """the heads' activated values as 16-bit steps (yolo_map_common.heads_from_u16), all heads in one array"""
    rows = sum(n * gh * gw for n, gh, gw, _ in heads)
    on = rng.random(rows) < frac if frac is not None else np.arange(rows) == rng.integers(rows)
    qs, at = [], 0
    for n, gh, gw, _ in heads:
        o = np.empty((n, 5 + classes, gh, gw), np.float64)
        o[:, 0:2] = rng.uniform(0.05, 0.95, (n, 2, gh, gw))
        o[:, 2:4] = np.clip(rng.normal(0.3, 0.4, (n, 2, gh, gw)), -1.9, 1.9) / 4 + 0.5
        m = on[at:at + n * gh * gw].reshape(n, gh, gw)
        o[:, 4] = np.where(m, rng.uniform(0.02, 1.0, (n, gh, gw)), rng.uniform(0.0, 0.004, (n, gh, gw)))
        o[:, 5:] = rng.uniform(0.0, 1.0, (n, classes, gh, gw)) ** 2
        qs.append(np.round(o * 65535).astype(np.uint16).reshape(-1))
        at += n * gh * gw
    return np.concatenate(qs)


def group_a(driver, tmp, arrays, meta):
    meta["a_cases"], worst = [], [1.0, 1.0]
    for name, heads, (net_w, net_h), classes, nms, frac in CASES_A:
        seed = 500
        while True:
            rng = np.random.default_rng([seed, len(name), classes, int(nms * 100)])
            q = make_heads(rng, heads, classes, frac)
            outs = heads_from_u16(q, [h[:3] for h in heads], classes)
            dets, idx, cand = survivors(driver, tmp, outs, heads, ANCH_A, net_w, net_h, classes, nms)
            gi, gp, equal = list_gaps(cand, nms)
            if gi > EPS_IOU and gp > EPS_PROB and not equal:
                break
            seed += 1
            if seed > 560:
                raise SystemExit("group A %s: no seed satisfies the conditions" % name)
        worst = [min(worst[0], gi), min(worst[1], gp)]
        live = (dets[:, 5:] > 0).any(1) if len(dets) else np.zeros(0, bool)
        arrays["a_%s_heads" % name] = q
        arrays["a_%s_index" % name] = idx              # every entry, in the order do_nms_sort left
        arrays["a_%s_live" % name] = np.nonzero(live)[0].astype(np.int32)      # ... those with a non-zero prob, whose rows are kept
        arrays["a_%s_dets" % name] = dets[live]
        meta["a_cases"].append(dict(name=name, heads=[[n, gh, gw, list(mask)] for n, gh, gw, mask in heads], net=[net_h, net_w], classes=classes, nms=nms,
                                    candidates=len(cand), survivors=[int((dets[:, 5 + k] > 0).sum()) for k in range(classes)], seed=seed,
                                    zero_ties=[int((cand[:, 5 + k] == 0).sum()) for k in range(classes)]))
    meta["a_gaps"] = dict(iou_to_nms=worst[0], prob_to_thresh=worst[1])


# ---------------------------------------------------------------------------------------------------- group B
def png(rgb):
    """an 8-bit RGB PNG of the uint8 [h, w, 3] array"""
    h, w = rgb.shape[:2]
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b"")


def conv_block(filters, size, stride, bn, act):
    return ("[convolutional]\n" + ("batch_normalize=1\n" if bn else "") +
            "filters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n" % (filters, size, stride, act))


def yolo_block(mask, anchors, classes):
    return ("[yolo]\nmask = %s\nanchors = %s\nclasses=%d\nnum=%d\njitter=.3\nignore_thresh = .7\ntruth_thresh = 1\nrandom=0\n\n"
            % (",".join(str(m) for m in mask), ",  ".join("%d,%d" % (a[0], a[1]) for a in anchors), classes, len(anchors)))


def make_net(rng, size, classes, two_heads, anchors):
    """(cfg text, weights file bytes, heads [(n, gh, gw, mask)]) of a tiny detector"""
    A = 3 * (5 + classes)
    cfg = "[net]\nbatch=1\nsubdivisions=1\nwidth=%d\nheight=%d\nchannels=3\n\n" % (size, size)
    convs = [(3, 8, 3, 2, True, "leaky"), (8, 8, 3, 2, True, "leaky"), (8, 8, 3, 2, True, "leaky"), (8, 8, 3, 2, True, "leaky"),
             (8, A, 1, 1, False, "linear")]
    for c in convs:
        cfg += conv_block(c[1], c[2], c[3], c[4], c[5])
    g = size // 16
    cfg += yolo_block((0, 1, 2), anchors, classes)
    heads = [(3, g, g, (0, 1, 2))]
    if two_heads:
        cfg += "[route]\nlayers = -3\n\n"
        convs += [(8, 8, 3, 2, True, "leaky"), (8, A, 1, 1, False, "linear")]
        cfg += conv_block(8, 3, 2, True, "leaky") + conv_block(A, 1, 1, False, "linear") + yolo_block((3, 4, 5), anchors, classes)
        heads.append((3, g // 2, g // 2, (3, 4, 5)))
    w = struct.pack("iii", 0, 2, 0) + struct.pack("q", 0)
    for cin, cout, k, _, bn, act in convs:
        if act == "linear":         # a head: per attribute scales, objectness biased low so a black frame detects nothing
            scale = np.tile(np.array([0.3, 0.3, 0.08, 0.08, 0.6] + [0.3] * classes, f32), 3)
            bias = np.tile(np.array([0, 0, 0, 0, -5.5] + [0.0] * classes, f32), 3)
            wt = rng.normal(0, 1, (cout, cin)).astype(f32) * scale[:, None]
            w += bias.tobytes() + wt.tobytes()
        else:
            wt = rng.normal(0, 1.0 / np.sqrt(cin * k * k), (cout, cin, k, k)).astype(f32)
            w += np.zeros(cout, f32).tobytes()
            if bn:
                w += rng.uniform(0.8, 1.2, cout).astype(f32).tobytes() + np.zeros(cout, f32).tobytes() + rng.uniform(0.05, 0.2, cout).astype(f32).tobytes()
            w += wt.tobytes()
    return cfg, w, heads


def make_frames(rng, F, size):
    """F frames of (size + 8) x (size + 5): noise in 8 x 8 blocks (which a PNG packs well), frame 0 black"""
    H, W = size + 5, size + 8
    frames = []
    for f in range(F):
        coarse = rng.integers(0, 256, ((H + 7) // 8, (W + 7) // 8, 3))
        fr = np.kron(coarse, np.ones((8, 8, 1)))[:H, :W].astype(np.uint8)
        frames.append(fr if f else np.zeros_like(fr))
    return frames


def parse_report(text):
    r = dict(ap=[float(v) for v in re.findall(r"ap = ([-0-9.naninf]+) %", text)])
    m = re.search(r"detections_count = (\d+), unique_truth_count = (\d+)", text)
    r["detections_count"], r["unique_truth_count"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"precision = ([-0-9.naninf]+), recall = ([-0-9.naninf]+), F1-score = ([-0-9.naninf]+)", text)
    r["precision"], r["recall"], r["f1"] = (float(m.group(i)) for i in (1, 2, 3))
    m = re.search(r"TP = (\d+), FP = (\d+), FN = (\d+), average IoU = ([-0-9.naninf]+) %", text)
    r["tp"], r["fp"], r["fn"], r["avg_iou"] = int(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(4))
    r["mAP"] = float(re.search(r"\(mAP\) = ([-0-9.naninf]+),", text).group(1))
    return r


def place_labels(rng, dets_per_frame, classes):
    """label rows per frame from the reference's detections: (rows per frame, facts)"""
    F = len(dets_per_frame)
    rows = [[] for _ in range(F)]
    dup = False
    for f in range(2, F):               # frame 0 is black (its label is never found), frame 1 has no label file
        d = dets_per_frame[f]
        for k in range(classes):
            live = d[d[:, 5 + k] > THRESH_CALC]
            live = live[np.argsort(-live[:, 5 + k])]
            if not len(live) or (k == 0 and f >= 8):
                continue                # class 0: six found truths here, four stray ones below = exactly 10
            b = live[0, :4].astype(np.float64)
            others = d[(d[:, 5 + k] > 0) & (d[:, 5 + k] < live[0, 5 + k])]
            jit = b * np.array([1, 1, 1 + rng.uniform(-.1, .1), 1 + rng.uniform(-.1, .1)])
            if not dup:                 # one truth that two detections claim: a box between two overlapping survivors
                for o in others:
                    if iou64(b, o[:4]) < 0.25:
                        continue
                    lo = np.minimum(b[:2] - b[2:] / 2, o[:2] - o[2:4] / 2)
                    hi = np.maximum(b[:2] + b[2:] / 2, o[:2] + o[2:4] / 2)
                    hull, mean = np.concatenate([(lo + hi) / 2, hi - lo]), (b + o[:4]) / 2
                    for t in np.linspace(0, 1, 11):
                        c = hull * t + mean * (1 - t)
                        if min(iou64(c, b), iou64(c, o[:4])) > 0.53:
                            jit, dup = c, True
                            break
                    if dup:
                        break
            b = jit
            rows[f].append((k,) + tuple(np.round(b, 6)))
    stray = lambda k: (k,) + tuple(np.round(np.concatenate([rng.uniform(0.05, 0.95, 2), rng.uniform(0.01, 0.03, 2)]), 6))
    n0 = sum(r[0] == 0 for fr in rows for r in fr)
    rows[0].append(stray(0))
    for i in range(10 - n0 - 1):
        rows[2 + i % (F - 2)].append(stray(0))
    if classes > 1:
        rows[3].append(stray(classes - 1))
    return rows, dup, n0


def group_b(driver, tmp, arrays, meta):
    meta["b_cases"], worst = [], [1.0, 1.0, 1.0]
    for name, size, classes, two, anchors, F in (("c1", 64, 1, False, [(12, 16), (24, 20), (32, 40)], 12),
                                                  ("c3", 64, 3, True, [(10, 12), (16, 28), (28, 20), (24, 44), (44, 32), (40, 48)], 12)):
        seed = 700
        while True:
            rng = np.random.default_rng([seed, classes])
            root = os.path.join(tmp, "b_%s_%d" % (name, seed))
            os.makedirs(os.path.join(root, "JPEGImages")), os.makedirs(os.path.join(root, "labels"))
            cfg, weights, heads = make_net(rng, size, classes, two, anchors)
            frames = make_frames(rng, F, size)
            paths = [os.path.join(root, "JPEGImages", "f%02d.png" % f) for f in range(F)]
            for p, fr in zip(paths, frames):
                open(p, "wb").write(png(fr))
            for fn, text in (("net.cfg", cfg), ("valid.txt", "\n".join(paths) + "\n"), ("obj.names", "".join("obj%d\n" % k for k in range(classes))),
                             ("obj.data", "classes = %d\nvalid = %s\nnames = %s\n" % (classes, os.path.join(root, "valid.txt"), os.path.join(root, "obj.names")))):
                open(os.path.join(root, fn), "w").write(text)
            open(os.path.join(root, "net.weights"), "wb").write(weights)
            dump = os.path.join(root, "rows.bin")
            subprocess.run([driver, "rows", os.path.join(root, "valid.txt"), os.path.join(root, "net.cfg"), os.path.join(root, "net.weights"), dump],
                           check=True, cwd=tmp, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            raw, at, preds, dets_pf, cands = open(dump, "rb").read(), 0, [], [], []
            for f in range(F):
                outs = []
                for n, gh, gw, _ in heads:
                    assert struct.unpack("iii", raw[at:at + 12]) == (n, gh, gw)
                    cnt = n * (5 + classes) * gh * gw
                    outs.append(np.frombuffer(raw[at + 12:at + 12 + 4 * cnt], f32).copy())
                    at += 12 + 4 * cnt
                preds.append(decode_pred(outs, heads, np.array(anchors, f32), size, size, classes))
                d, _, cand = survivors(driver, tmp, outs, heads, np.array(anchors, f32), size, size, classes, NMS)
                dets_pf.append(d), cands.append(cand)
            rows, dup, found0 = place_labels(rng, dets_pf, classes)
            for f in range(F):
                if f != 1:
                    open(os.path.join(root, "labels", "f%02d.txt" % f), "w").write("".join("%d %.6f %.6f %.6f %.6f\n" % r for r in rows[f]))
            # the margins, from the reference's boxes in float64
            gi = gp = gl = 1.0
            allp = []
            for f in range(F):
                a, b, _ = list_gaps(cands[f], NMS)
                gi, gp = min(gi, a), min(gp, b)
                d = dets_pf[f]
                p = d[:, 5:].astype(np.float64)
                allp.append(p[p > 0])
                if (p > 0).any():
                    gp = min(gp, float(np.abs(p[p > 0] - THRESH_CALC).min()))
                if rows[f] and len(d):
                    lab = np.array(rows[f], np.float64)
                    m = iou64(d[:, None, :4], lab[None, :, 1:].astype(f32))
                    gi = min(gi, float(np.nanmin(np.abs(m - IOU_THRESH))))
                    for k in range(classes):
                        mk = m[:, lab[:, 0] == k]
                        if mk.shape[1] > 1:
                            s = np.sort(mk, 1)
                            top = s[:, -1] > IOU_THRESH
                            if top.any():
                                gl = min(gl, float((s[top, -1] - s[top, -2]).min()))
            allp = np.concatenate(allp)
            equal = len(np.unique(allp)) != len(allp)
            none_in_black = len(dets_pf[0]) == 0
            text = subprocess.run([driver, "map", os.path.join(root, "obj.data"), os.path.join(root, "net.cfg"), os.path.join(root, "net.weights"),
                                   "%.2f" % THRESH_CALC], check=True, cwd=tmp, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode()
            rep = parse_report(text)
            ok = gi > EPS_IOU and gp > EPS_PROB and gl > 1e-6 and not equal and dup and none_in_black and found0 >= 3 and rep["tp"] >= 3
            if os.environ.get("YOLO_MAP_GOLDEN_VERBOSE"):
                print(name, seed, dict(gi=gi, gp=gp, gl=gl, equal=equal, dup=dup, black=len(dets_pf[0]), found0=found0, report=rep,
                                       dets=[len(d) for d in dets_pf]), file=sys.stderr)
            if ok:
                break
            seed += 1
            if seed > 760:
                raise SystemExit("group B %s: no seed satisfies the conditions" % name)
        worst = [min(worst[0], gi), min(worst[1], gp), min(worst[2], gl)]
        lab = [r for fr in rows for r in fr]
        arrays["b_%s_labels" % name] = np.array(lab, f32).reshape(-1, 5)
        arrays["b_%s_first" % name] = np.cumsum([0] + [len(fr) for fr in rows]).astype(np.int32)
        arrays["b_%s_pred" % name] = np.stack(preds)
        arrays["b_%s_weights" % name] = np.frombuffer(weights, np.uint8)
        for f, fr in enumerate(frames):
            arrays["b_%s_png%02d" % (name, f)] = np.frombuffer(png(fr), np.uint8)
        meta["b_cases"].append(dict(name=name, classes=classes, net=[size, size], heads=[[n, gh, gw] for n, gh, gw, _ in heads], frames=F,
                                    cfg=cfg, report=rep, seed=seed, no_label_frame=1,
                                    no_detection_frame=0, class0_truths=10, class0_truths_with_a_detection=found0,
                                    truth_classes_count=[int(sum(r[0] == k for r in lab)) for k in range(classes)]))
    meta["b_gaps"] = dict(iou_to_threshold=worst[0], prob_to_threshold=worst[1], label_tie=worst[2])


def main():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    arrays, meta = {}, {"reference_ran": ["make_network", "make_yolo_layer", "get_network_boxes", "do_nms_sort", "parse_network_cfg_custom",
                                          "load_weights", "fuse_conv_batchnorm", "load_image_color", "resize_image", "network_predict",
                                          "validate_detector_map"],
                        "restated": ["pred: the detector's decode of the heads' activated values, float32 numpy",
                                     "the IoUs and margins the conditions test (numpy float64 of the reference's boxes)"],
                        "conditions": {"iou_to_threshold": EPS_IOU, "prob_to_threshold": EPS_PROB, "equal_probs": 0, "label_tie": 1e-6},
                        "exempt_cases": 0, "thresh": THRESH, "nms": NMS, "iou_thresh": IOU_THRESH, "thresh_calc": THRESH_CALC}
    with tempfile.TemporaryDirectory() as tmp:
        driver = os.path.join(tmp, "yolo_map_ref_driver")
        subprocess.check_call(["gcc", "-O2", "-w", "-I", SRC, os.path.join(ROOT, "tools", "yolo_map_ref_driver.c"), "-o", driver,
                               "-L", os.path.dirname(LIB), "-ldarknet_ref", "-Wl,-rpath," + os.path.dirname(LIB), "-lm"])
        group_a(driver, tmp, arrays, meta)
        group_b(driver, tmp, arrays, meta)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    save_npz(OUT, arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    print(json.dumps({k: meta[k] for k in ("a_gaps", "b_gaps")}))
    print(json.dumps([c["report"] for c in meta["b_cases"]]))


if __name__ == "__main__":
    main()
