"""What the detector-validation tests share (test_yolo_map_host.py, test_gpu_yolo_map.py): the golden archive with its
meta, the head values of its box-list cases as ``pred``, seeded predictions with a chosen number of candidates, and a
plain-Python statement of the three calls for the seeded cases."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ANCHORS = np.array([10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119], f32).reshape(6, 2)


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "yolo_map.npz"))
    out = {k: g[k] for k in g.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def meta():
    return json.loads(bytes(golden()["meta"]).decode())


def heads_from_u16(q, heads, classes):
    """the activated head values the archive keeps as 16-bit steps: per head float32 [n, 5 + classes, gh, gw]; x, y,
    objectness and classes are q / 65535, the two size entries (q / 65535 - .5) * 4"""
    outs, at = [], 0
    for n, gh, gw in heads:
        cnt = n * (5 + classes) * gh * gw
        o = (q[at:at + cnt].astype(f32) / f32(65535)).reshape(n, 5 + classes, gh, gw)
        o[:, 2:4] = (o[:, 2:4] - f32(0.5)) * f32(4)
        outs.append(o)
        at += cnt
    return outs


def decode_pred(outs, heads, anchors, net_w, net_h, classes):
    """the detector's decode of activated head values (Darknet's layout) in float32: [rows, 5 + classes], rows ordered
    head, anchor, gy, gx; ``heads`` = [(n, gh, gw, mask)]"""
    rows = []
    for o, (n, gh, gw, mask) in zip(outs, heads):
        o = o.reshape(n, 5 + classes, gh, gw)
        sx, sy = f32(net_w // gw), f32(net_h // gh)
        gx, gy = np.meshgrid(np.arange(gw, dtype=f32), np.arange(gh, dtype=f32))
        for a in range(n):
            aw, ah = anchors[mask[a]]
            r = np.empty((gh, gw, 5 + classes), f32)
            r[..., 0] = (o[a, 0] + gx) * sx
            r[..., 1] = (o[a, 1] + gy) * sy
            r[..., 2] = (np.exp(o[a, 2]).astype(f32) * (aw / sx)) * sx
            r[..., 3] = (np.exp(o[a, 3]).astype(f32) * (ah / sy)) * sy
            r[..., 4:] = np.moveaxis(o[a, 4:], 0, -1)
            rows.append(r.reshape(-1, 5 + classes))
    return np.concatenate(rows).astype(f32)


def table(heads):
    from betapose_amd.yolo_map import heads_table
    return heads_table([h[:3] for h in heads])


def a_case(c):
    """group A case ``c`` of the meta: (pred [1, rows, attrs], head table, net_size, classes, nms)"""
    g = golden()
    heads = [tuple(h[:3]) + (tuple(h[3]),) for h in c["heads"]]
    outs = heads_from_u16(np.array(g["a_%s_heads" % c["name"]]), [h[:3] for h in heads], c["classes"])
    pred = decode_pred(outs, heads, ANCHORS, c["net"][1], c["net"][0], c["classes"])
    return pred[None], table(heads), tuple(c["net"]), c["classes"], c["nms"]


def b_case(c):
    """group B case ``c``: (pred [F, rows, attrs], labels, first, head table, net_size, classes)"""
    g = golden()
    n = c["name"]
    return (np.array(g["b_%s_pred" % n]), np.array(g["b_%s_labels" % n]), np.array(g["b_%s_first" % n]),
            table([tuple(h) for h in c["heads"]]), tuple(c["net"]), c["classes"])


def write_b_tree(c, root):
    """the validation tree of group B case ``c`` under ``root``: frames, label files, cfg, weights, names, list, .data;
    returns the .data path"""
    g = golden()
    n = c["name"]
    os.makedirs(os.path.join(root, "JPEGImages")), os.makedirs(os.path.join(root, "labels"))
    labels, first = np.array(g["b_%s_labels" % n]), np.array(g["b_%s_first" % n])
    paths = []
    for f in range(c["frames"]):
        paths.append(os.path.join(root, "JPEGImages", "f%02d.png" % f))
        with open(paths[-1], "wb") as fh:
            fh.write(bytes(g["b_%s_png%02d" % (n, f)]))
        if f != c["no_label_frame"]:
            with open(os.path.join(root, "labels", "f%02d.txt" % f), "w") as fh:
                fh.write("".join("%d %.6f %.6f %.6f %.6f\n" % (r[0], r[1], r[2], r[3], r[4]) for r in labels[first[f]:first[f + 1]]))
    files = (("net.cfg", c["cfg"]), ("valid.txt", "\n".join(paths) + "\n"), ("obj.names", "".join("obj%d\n" % k for k in range(c["classes"]))),
             ("obj.data", "classes = %d\n# a comment\nvalid = %s\nnames = %s\n" % (c["classes"], os.path.join(root, "valid.txt"),
                                                                                 os.path.join(root, "obj.names"))))
    for fn, text in files:
        with open(os.path.join(root, fn), "w") as fh:
            fh.write(text)
    with open(os.path.join(root, "net.weights"), "wb") as fh:
        fh.write(bytes(g["b_%s_weights" % n]))
    return os.path.join(root, "obj.data")


# ---------------------------------------------------------------------------------------------------- seeded inputs
SEED_HEADS = [(3, 13, 13), (3, 26, 26), (3, 6, 4)]      # 2 607 rows
SEED_NET = (416, 416)


def seeded_pred(seed, counts, classes, heads=SEED_HEADS, net=SEED_NET):
    """pred [len(counts), rows, 5 + classes] with exactly counts[b] rows above objectness .005 in image b, boxes that
    overlap in clusters, distinct probs"""
    rng = np.random.default_rng([seed, classes] + list(counts))
    rows = sum(n * gh * gw for n, gh, gw in heads)
    pred = np.empty((len(counts), rows, 5 + classes), f32)
    for b, cnt in enumerate(counts):
        centers = rng.uniform(40, net[1] - 40, (12, 2))
        c = centers[rng.integers(0, 12, rows)] + rng.normal(0, 14, (rows, 2))
        pred[b, :, 0:2] = c
        pred[b, :, 2:4] = rng.uniform(30, 90, (rows, 2))
        obj = rng.uniform(0.0, 0.004, rows)
        on = rng.permutation(rows)[:cnt]
        obj[on] = rng.uniform(0.05, 1.0, cnt)
        pred[b, :, 4] = obj
        pred[b, :, 5:] = rng.uniform(0.0, 1.0, (rows, classes)) ** 2
    return pred, table(heads)


def seeded_labels(seed, pred, classes, per_image=4):
    """labels near some candidates of every image, and a few stray ones: (labels [M, 5], first [B + 1])"""
    rng = np.random.default_rng([seed, 77])
    rows, first = [], [0]
    for b in range(len(pred)):
        on = np.nonzero(pred[b, :, 4] > 0.3)[0]
        for r in on[:per_image]:
            x, y, w, h = pred[b, r, :4] / f32(SEED_NET[1])
            rows.append((rng.integers(0, classes), x + rng.uniform(-.01, .01), y, w * rng.uniform(.9, 1.1), h))
        if b % 2 == 0:
            rows.append((rng.integers(0, classes), rng.uniform(.1, .9), rng.uniform(.1, .9), .02, .02))
        first.append(len(rows))
    return np.array(rows, f32).reshape(-1, 5), np.array(first, np.int32)


def seeded_records(seed, D, classes, truths, images=50):
    """D records as map_match writes them, with duplicate claims and equal probs across images: (rec [D, 6] float32,
    truth_classes_count, img_stats [images, 3])"""
    rng = np.random.default_rng([seed, D, classes])
    rec = np.zeros((D, 6), f32)
    rec[:, 0] = (rng.integers(1, 4000, D) / 4000.0).astype(f32)     # ties in p on purpose
    img = np.sort(rng.integers(0, images, D)).astype(np.int32)
    rec[:, 1] = img.view(f32)
    cls = rng.integers(0, classes, D).astype(np.int32)
    rec[:, 2] = cls.view(f32)
    truth = np.where(rng.random(D) < 0.4, rng.integers(0, max(truths, 1), D), -1).astype(np.int32)
    if truths == 0:
        truth[:] = -1
    rec[:, 3] = truth.view(f32)
    rec[:, 4] = rng.uniform(0.5, 1, D).astype(f32)
    pos = np.zeros(D, np.int32)
    for i in range(1, D):
        pos[i] = pos[i - 1] + 1 if img[i] == img[i - 1] else 0
    rec[:, 5] = pos.view(f32)
    tcc = np.bincount(rng.integers(0, classes, truths), minlength=classes).astype(np.int32) if truths else np.zeros(classes, np.int32)
    st = np.stack([rng.integers(0, 5, images), rng.integers(0, 9, images), rng.uniform(0, 4, images)], 1).astype(np.float64)
    return rec, tcc, st


# ---------------------------------------------------------------------------------------------------- plain statements
def iou32(a, b):
    """box_iou in float32 steps, as box.c"""
    def ov(x1, w1, x2, w2):
        l = max(f32(x1 - w1 / f32(2)), f32(x2 - w2 / f32(2)))
        r = min(f32(x1 + w1 / f32(2)), f32(x2 + w2 / f32(2)))
        return f32(r - l)
    w, h = ov(a[0], a[2], b[0], b[2]), ov(a[1], a[3], b[1], b[3])
    inter = f32(0) if (w < 0 or h < 0) else f32(w * h)
    with np.errstate(invalid="ignore", divide="ignore"):
        return f32(inter / f32(f32(f32(a[2] * a[3]) + f32(b[2] * b[3])) - inter))


def reduce_plain(rec, tcc, classes, truths, img_stats):
    """detector.c:774-876 with the stable tie rule, in Python: (ap [classes], stats dict)"""
    D = len(rec)
    p, img, cls, truth, pos = rec[:, 0], rec[:, 1].view(np.int32), rec[:, 2].view(np.int32), rec[:, 3].view(np.int32), rec[:, 5].view(np.int32)
    order = sorted(range(D), key=lambda i: (-float(p[i]), int(img[i]), int(pos[i]), i))
    flags = set()
    tp, fp = np.zeros(classes, int), np.zeros(classes, int)
    best = np.zeros((classes, 11))
    for i in order:
        if truth[i] >= 0:
            if truth[i] not in flags:
                flags.add(int(truth[i]))
                tp[cls[i]] += 1
        else:
            fp[cls[i]] += 1
        for c in range(classes):
            fn = tcc[c] - tp[c]
            pr = tp[c] / (tp[c] + fp[c]) if tp[c] + fp[c] > 0 else 0.0
            rc = tp[c] / (tp[c] + fn) if tp[c] + fn > 0 else 0.0
            for q in range(11):
                if rc >= q * 0.1 and pr > best[c, q]:
                    best[c, q] = pr
    ap = np.array([sum(best[c]) / 11 for c in range(classes)])
    return ap, dict(mAP=sum(ap) / classes, tp=int(img_stats[:, 0].sum()), fp=int(img_stats[:, 1].sum()))
