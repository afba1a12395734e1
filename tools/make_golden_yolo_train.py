#!/usr/bin/env python3
"""Generate tests/golden/yolo_train.npz by running the REFERENCE's own Darknet C code (build machine only; nothing of
the reference is copied).  ``oracle/_ref/libdarknet_ref.so`` (oracle/Makefile) is loaded through ctypes for

  images   ``crop_image`` -> ``resize_image`` -> ``flip_image`` -> ``distort_image`` on two noise frames (37 x 70 and
           48 x 64, with a few black and grey pixels) at 24 x 16 and 32 x 32 (net_h x net_w): four whole chains and one
           case per stage alone.  ``rgb_to_hsv`` on a copy gives the hue before wrapping for the condition below.
  truths   ``srand(s)``, ``random_gen()``'s draws recorded, ``srand(s)`` again, ``fill_truth_detection`` on temporary
           label files: 0, 1, 5 and 95 boxes, a box the crop pushes out, one smaller than a pixel, ``id >= classes``, an
           ``x = y = 0`` line, flip.

and for ``forward_yolo_layer`` the project's own driver tools/yolo_layer_ref_driver.c is compiled against the
reference's headers into a temporary directory and run once per loss case (grids 3 x 2, 5 x 7 and 13 x 13 as w x h,
B = 2, n = 3, total = 9, every mask triple, classes 1 and 3, ignore_thresh .5 / .7, truth_thresh 1 / .9); its log line is
kept as text.

Restated here (``meta["restated"]``): the frame's ``u8 / 255`` (load_image needs a file), the rows kept (counted from
the truth the reference filled), and the IoUs the conditions test (numpy float64 from the reference's l.output).

Conditions, enforced by re-seeding until the reference alone stays inside them, with no exempt case: no best IoU within
1e-4 of ignore_thresh, truth_thresh, .5 or .75; the best and second-best anchor IoU of every truth differ by more than
1e-6; no truth.x * w or truth.y * h within 1e-4 of an integer; no hue before wrapping within 1e-5 of 0 or 1; and one more, so that
"the non-zero deltas lie where the reference's do" asks nothing of a rounding: no non-zero delta of the reference below 1e-5
in magnitude (the cells engineered to pass truth_thresh predict their truth with an offset, not exactly).

The archive is written with fixed time stamps: running this twice gives the same bytes.

Usage: python tools/make_golden_yolo_train.py
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_shims  # noqa: E402  (only for where the reference lies)
from betapose_amd.train_data import save_npz  # noqa: E402

SRC = os.path.join(ref_shims.REF, "train_YOLO", "src")
LIB = os.path.join(ROOT, "oracle", "_ref", "libdarknet_ref.so")
OUT = os.path.join(ROOT, "tests", "golden", "yolo_train.npz")
ANCHORS = np.array([10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326], np.float32).reshape(9, 2)
NET = 416
MAX_BOXES = 90
EPS_IOU, EPS_ANCHOR, EPS_CELL, EPS_HUE, EPS_DELTA = 1e-4, 1e-6, 1e-4, 1e-5, 1e-5


class Image(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]


def load_ref():
    L = C.CDLL(LIB)
    L.crop_image.restype = Image
    L.crop_image.argtypes = [Image, C.c_int, C.c_int, C.c_int, C.c_int]
    L.resize_image.restype = Image
    L.resize_image.argtypes = [Image, C.c_int, C.c_int]
    for name in ("flip_image", "rgb_to_hsv"):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = [Image]
    L.distort_image.restype = None
    L.distort_image.argtypes = [Image, C.c_float, C.c_float, C.c_float]
    L.free_image.restype = None
    L.free_image.argtypes = [Image]
    L.random_gen.restype = C.c_uint
    L.fill_truth_detection.restype = None
    L.fill_truth_detection.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_float, C.c_float,
                                       C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
    return L


def as_image(a):
    """an Image over the float32 [3, h, w] array ``a`` (which must outlive it)"""
    return Image(a.shape[2], a.shape[1], 3, a.ctypes.data_as(C.POINTER(C.c_float)))


def to_array(im):
    return np.ctypeslib.as_array(im.data, shape=(im.c, im.h, im.w)).copy()


# ---------------------------------------------------------------------------------------------------- images
def make_frames(rng):
    frames = []
    for h, w in ((37, 70), (48, 64)):
        f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        f[3, 5] = 0                     # black: max == 0
        f[4:6, 7] = 128                 # grey: hue 0 / 0
        f[h - 1, w - 1] = (255, 255, 255)
        f[10, 10] = (200, 200, 17)      # r == g == max
        frames.append(f)
    return frames


IMAGE_CASES = [
    # name, frame, (net_h, net_w), (pleft, ptop, swidth, sheight), flip, hsv
    ("inside", 0, (24, 16), (5, 4, 50, 29), 0, (0.07, 1.31, 0.81)),
    ("past_all_edges", 0, (32, 32), (-9, -6, 90, 50), 1, (-0.12, 0.77, 1.27)),
    ("left_in_right_out", 1, (24, 16), (11, 3, 60, 40), 1, None),
    ("plain", 1, (32, 32), (2, 2, 57, 41), 0, None),
    ("stage_crop", 1, (24, 16), (-3, 30, 16, 24), 0, None),
    ("stage_resize", 1, (24, 16), (0, 0, 64, 48), 0, None),
    ("stage_flip", 1, (24, 16), (20, 10, 16, 24), 1, None),
    ("stage_distort", 1, (24, 16), (20, 10, 16, 24), 0, (0.21, 1.45, 0.7)),
    ("hue_wraps_down", 0, (24, 16), (30, 5, 16, 24), 0, (-0.28, 1 / 1.2, 1.4)),
]


def run_image_case(L, frame, net, crop, flip, hsv):
    """the reference's chain; returns (result [3, net_h, net_w], min distance of a hue before wrapping to 0 or 1)"""
    orig = (frame.astype(np.float64) / 255.0).astype(np.float32).transpose(2, 0, 1).copy()      # load_image's u8 / 255.
    cropped = L.crop_image(as_image(orig), *crop)
    sized = L.resize_image(cropped, net[1], net[0])
    if flip:
        L.flip_image(sized)
    gap = 1.0
    if hsv is not None:
        probe = to_array(sized)
        L.rgb_to_hsv(as_image(probe))
        hue = probe[0].astype(np.float64) + np.float32(hsv[0])
        hue = hue[np.isfinite(hue)]
        gap = float(np.minimum(np.abs(hue), np.abs(hue - 1)).min())
        L.distort_image(sized, *hsv)
    out = to_array(sized)
    L.free_image(cropped)
    L.free_image(sized)
    return out, gap


# ---------------------------------------------------------------------------------------------------- truths
def f32s(v):
    return "%.9g" % float(np.float32(v))


def label_lines(rng, n, classes):
    rows = []
    for _ in range(n):
        w, h = rng.uniform(0.05, 0.3, 2)
        rows.append([int(rng.integers(0, classes)), rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), w, h])
    return rows


def truth_cases(rng):
    """name -> (rows, classes, flip, (dx, dy, sx, sy))"""
    geom = lambda pl, pt, sw, sh, ow=640, oh=480: tuple(float(v) for v in (
        np.float32(np.float32(pl) / np.float32(ow)) / (np.float32(sw) / np.float32(ow)),
        np.float32(np.float32(pt) / np.float32(oh)) / (np.float32(sh) / np.float32(oh)),
        np.float32(1.0 / float(np.float32(sw) / np.float32(ow))), np.float32(1.0 / float(np.float32(sh) / np.float32(oh)))))
    five = label_lines(rng, 5, 1)
    five[0][1:3] = [0.04, 0.5]          # the crop pushes it out of the image (x <= 0 after the shift)
    five[1][3:5] = [0.001, 0.001]       # smaller than a pixel
    five[2][0] = 1                      # id >= classes
    zero = label_lines(rng, 4, 3)
    zero[1][1:3] = [0.0, 0.0]           # the x = y = 0 marker
    many = label_lines(rng, 95, 2)
    for i in range(0, 95, 9):
        many[i][3:5] = [0.0005, 0.2]    # filtered rows among the first 90: truncation comes first
    return {
        "none": ([], 1, 0, geom(10, -20, 600, 500)),
        "one": (label_lines(rng, 1, 1), 1, 0, geom(-30, 12, 700, 430)),
        "five": (five, 1, 0, geom(120, 10, 500, 460)),
        "zero_marker_flip": (zero, 3, 1, geom(-50, 30, 660, 420)),
        "ninety_five_flip": (many, 2, 1, geom(20, -15, 610, 505)),
    }


def run_truth_case(L, tmp, name, rows, classes, flip, geom, seed):
    img = os.path.join(tmp, name + ".jpg")
    with open(os.path.join(tmp, name + ".txt"), "w") as f:
        for r in rows:
            f.write("%d %s %s %s %s\n" % (r[0], f32s(r[1]), f32s(r[2]), f32s(r[3]), f32s(r[4])))
    n = len(rows)
    L.srand(seed)
    draws = [int(L.random_gen()) for _ in range(n)]
    L.srand(seed)
    truth = np.zeros((MAX_BOXES, 5), np.float32)
    L.fill_truth_detection(img.encode(), MAX_BOXES, truth.ctypes.data_as(C.POINTER(C.c_float)), classes, flip, *geom, 0, NET, NET)
    labels = np.array([[r[0]] + [float(np.float32(v)) for v in r[1:]] for r in rows], np.float32).reshape(-1, 5)
    swap = np.array([d % n for d in draws], np.int32)
    return labels, swap, truth


# ---------------------------------------------------------------------------------------------------- loss
def logit(p):
    return float(np.log(p / (1 - p)))


def iou64(a, b):
    """box_iou in float64 on [..., 4] arrays (x, y, w, h)"""
    def ov(x1, w1, x2, w2):
        return np.minimum(x1 + w1 / 2, x2 + w2 / 2) - np.maximum(x1 - w1 / 2, x2 - w2 / 2)
    w, h = ov(a[..., 0], a[..., 2], b[..., 0], b[..., 2]), ov(a[..., 1], a[..., 3], b[..., 1], b[..., 3])
    inter = np.where((w < 0) | (h < 0), 0.0, w * h)
    return inter / (a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter)


def make_truth(rng, w, h, classes, full_second):
    """[2, MAX_BOXES, 5]: image 0 holds one truth per head and two pairs in one cell with the same best anchor (the same
    class, and different classes when there are several); image 1 is empty or holds MAX_BOXES truths"""
    def box(anchor, cell=None, cls=None):
        aw, ah = ANCHORS[anchor] / NET
        s = rng.uniform(0.85, 1.18, 2)
        i, j = (rng.integers(0, w), rng.integers(0, h)) if cell is None else cell
        fx, fy = rng.uniform(0.15, 0.85, 2)
        return [(i + fx) / w, (j + fy) / h, aw * s[0], ah * s[1], rng.integers(0, classes) if cls is None else cls]
    t = np.zeros((2, MAX_BOXES, 5), np.float32)
    rows = [box(1), box(4), box(7)]
    cell = (int(rng.integers(0, w)), int(rng.integers(0, h)))
    for a in (0, 3, 8):
        rows += [box(a, cell, 0), box(a, cell, 0 if classes == 1 else 1)]
    cell2 = ((cell[0] + 1) % w, cell[1])
    rows += [box(5, cell2, classes - 1), box(5, cell2, classes - 1)]
    t[0, :len(rows)] = rows
    if full_second:
        t[1] = [box(int(rng.integers(0, 9))) for _ in range(MAX_BOXES)]
    return t


def make_x(rng, B, n, classes, h, w, truth, mask, engineer):
    x = (np.round(rng.normal(0, 1.2, (B, n, 5 + classes, h, w)) * 64) / 64).astype(np.float32)
    if engineer:        # a cell whose prediction overlaps a truth by more than .9: the truth_thresh branch runs
        for k in (0, 1):
            tx, ty, tw, th = (float(v) for v in truth[0, k, :4])
            i, j = int(tx * w), int(ty * h)
            aw, ah = ANCHORS[mask[k % n]]
            x[0, k % n, :4, j, i] = (logit(tx * w - i) + 0.04, logit(ty * h - j) - 0.03, np.log(tw * NET / aw) + 0.02, np.log(th * NET / ah) - 0.015)
    return x.reshape(B, n * (5 + classes), h, w)


def run_driver(driver, tmp, x, truth, mask, classes, ignore, thresh):
    B, _, h, w = x.shape
    n = len(mask)
    inp, out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([B, n, 9, classes, h, w, NET, NET, MAX_BOXES], np.int32).tobytes())
        f.write(np.array([ignore, thresh], np.float32).tobytes())
        f.write(np.asarray(mask, np.int32).tobytes() + ANCHORS.tobytes() + truth.tobytes() + x.tobytes())
    r = subprocess.run([driver, inp, out], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, stdin=subprocess.DEVNULL, check=True)
    raw = np.fromfile(out, np.float32)
    return raw[:x.size].reshape(x.shape), raw[x.size:2 * x.size].reshape(x.shape), raw[-1], r.stdout.decode().strip()


def loss_gaps(act, truth, mask, classes, ignore, thresh):
    """(smallest distance of a best IoU to a threshold, smallest best / second anchor gap, smallest distance of
    truth.x * w or truth.y * h to an integer, cells above truth_thresh) from the reference's l.output"""
    B, _, h, w = act.shape
    n = len(mask)
    a = act.reshape(B, n, 5 + classes, h, w).astype(np.float64)
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    aw = ANCHORS[mask, 0].astype(np.float64)[None, :, None, None]
    ah = ANCHORS[mask, 1].astype(np.float64)[None, :, None, None]
    pred = np.stack([(ii + a[:, :, 0]) / w, (jj + a[:, :, 1]) / h, np.exp(a[:, :, 2]) * aw / NET, np.exp(a[:, :, 3]) * ah / NET], -1)
    gap_iou, gap_anchor, gap_cell, above = 1.0, 1.0, 1.0, 0
    marks = np.array([ignore, thresh, 0.5, 0.75])
    for b in range(B):
        rows = []
        for t in truth[b]:
            if t[0] == 0:
                break
            rows.append(t.astype(np.float64))
        if not rows:
            continue
        rows = np.array(rows)
        ious = iou64(pred[b][..., None, :], rows[:, :4])        # [n, h, w, T]
        best = ious.max(-1)
        gap_iou = min(gap_iou, float(np.abs(best[..., None] - marks).min()))
        above += int((best > thresh).sum())
        zero = np.zeros(9)
        anchors = np.stack([zero, zero, ANCHORS[:, 0] / np.float64(NET), ANCHORS[:, 1] / np.float64(NET)], -1)
        for t in rows:
            shifted = np.array([0, 0, t[2], t[3]])
            s = np.sort(iou64(anchors, shifted))
            gap_anchor = min(gap_anchor, float(s[-1] - s[-2]))
            fx, fy = t[0] * w, t[1] * h
            gap_cell = min(gap_cell, abs(fx - round(fx)), abs(fy - round(fy)))
            best_n = int(np.argmax(iou64(anchors, shifted)))
            if best_n in list(mask):
                m = list(mask).index(best_n)
                iou = float(iou64(pred[b, m, int(fy), int(fx)], t[:4]))
                gap_iou = min(gap_iou, float(np.abs(iou - marks[2:]).min()))
    return gap_iou, gap_anchor, gap_cell, above


MASKS = ((0, 1, 2), (3, 4, 5), (6, 7, 8))


def loss_case_list():
    """(name, w, h, classes, mask index, ignore_thresh, truth_thresh, image 1 full)"""
    cases = []
    for m in range(3):
        for classes in (1, 3):
            for k, (ig, th) in enumerate(((0.5, 1.0), (0.7, 0.9))):
                cases.append(("g3x2_c%d_m%d_t%d" % (classes, m, k), 3, 2, classes, m, ig, th, m == 2 and k == 1))
            ig, th = ((0.7, 1.0), (0.5, 0.9))[(m + classes) % 2]
            cases.append(("g5x7_c%d_m%d" % (classes, m), 5, 7, classes, m, ig, th, m == 0))
    cases.append(("g13x13_c1_m2", 13, 13, 1, 2, 0.7, 1.0, True))
    return cases


def main():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    L = load_ref()
    arrays, meta = {}, {"reference_ran": ["crop_image", "resize_image", "flip_image", "distort_image", "rgb_to_hsv", "random_gen",
                                          "fill_truth_detection", "correct_boxes", "make_yolo_layer", "forward_yolo_layer"],
                        "restated": ["u8 / 255 of the frames", "kept = rows the reference filled",
                                     "the IoUs the conditions test (numpy float64 from the reference's l.output)"],
                        "conditions": {"iou_to_threshold": EPS_IOU, "anchor_gap": EPS_ANCHOR, "cell_to_integer": EPS_CELL,
                                       "hue_to_wrap": EPS_HUE, "delta_to_zero": EPS_DELTA}, "exempt_cases": 0, "net": NET, "max_boxes": MAX_BOXES}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)                   # fill_truth_detection appends to bad_label.list in the working directory
        devnull = os.open(os.devnull, os.O_RDONLY)
        os.dup2(devnull, 0)             # ... and waits on getchar() after an id >= classes
        try:
            # images
            seed = 100
            while True:
                rng = np.random.default_rng(seed)
                frames = make_frames(rng)
                outs = [run_image_case(L, frames[c[1]], c[2], c[3], c[4], c[5]) for c in IMAGE_CASES]
                if min(g for _, g in outs) > EPS_HUE:
                    break
                seed += 1
            meta["image_seed"], meta["image_hue_gap"] = seed, min(g for _, g in outs)
            arrays["frame0"], arrays["frame1"] = frames
            meta["image_cases"] = []
            for c, (o, _) in zip(IMAGE_CASES, outs):
                arrays["img_" + c[0]] = o
                meta["image_cases"].append(dict(name=c[0], frame=c[1], net=c[2], crop=c[3], flip=c[4], hsv=c[5]))
            # truths
            rng = np.random.default_rng(200)
            meta["truth_cases"] = []
            for k, (name, (rows, classes, flip, geom)) in enumerate(truth_cases(rng).items()):
                labels, swap, truth = run_truth_case(L, tmp, name, rows, classes, flip, geom, 7 + k)
                arrays["truth_%s_labels" % name], arrays["truth_%s_swap" % name], arrays["truth_%s_out" % name] = labels, swap, truth
                meta["truth_cases"].append(dict(name=name, classes=classes, flip=flip, geom=geom, kept=int((truth[:, 0] != 0).sum())))
            # loss
            driver = os.path.join(tmp, "yolo_layer_ref_driver")
            subprocess.check_call(["gcc", "-O2", "-w", "-I", SRC, os.path.join(ROOT, "tools", "yolo_layer_ref_driver.c"), "-o", driver,
                                   "-L", os.path.dirname(LIB), "-ldarknet_ref", "-Wl,-rpath," + os.path.dirname(LIB), "-lm"])
            meta["loss_cases"] = []
            shared = {}
            worst = [1.0, 1.0, 1.0, 1.0]
            for name, w, h, classes, m, ig, th, full in loss_case_list():
                seed = 300
                while True:
                    rng = np.random.default_rng([seed, w, h, classes, m, int(full), int(th * 10)])
                    truth = make_truth(rng, w, h, classes, full)
                    x = make_x(rng, 2, 3, classes, h, w, truth, MASKS[m], th < 1)
                    delta, act, cost, line = run_driver(driver, tmp, x, truth, MASKS[m], classes, ig, th)
                    gi, ga, gc, above = loss_gaps(act, truth, MASKS[m], classes, ig, th)
                    gd = float(np.abs(delta[delta != 0]).min())
                    if gi > EPS_IOU and ga > EPS_ANCHOR and gc > EPS_CELL and gd > EPS_DELTA and (th >= 1 or above > 0):
                        break
                    seed += 1
                worst = [min(a, b) for a, b in zip(worst, (gi, ga, gc, gd))]
                arrays["loss_%s_x" % name], arrays["loss_%s_truth" % name] = x, truth[:, :, :]
                arrays["loss_%s_delta" % name], arrays["loss_%s_act" % name] = delta, act
                meta["loss_cases"].append(dict(name=name, w=w, h=h, classes=classes, mask=MASKS[m], ignore_thresh=ig, truth_thresh=th,
                                               cost=float(cost), line=line, seed=seed, cells_above_truth_thresh=above))
            meta["loss_gaps"] = dict(iou_to_threshold=worst[0], anchor_gap=worst[1], cell_to_integer=worst[2], delta_to_zero=worst[3])
        finally:
            os.chdir(cwd)
    arrays["anchors"] = ANCHORS
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    save_npz(OUT, arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    print(json.dumps({k: meta[k] for k in ("image_hue_gap", "loss_gaps")}))


if __name__ == "__main__":
    main()
