"""What the detector-training tests share (test_yolo_train_host.py, test_gpu_yolo_train.py): the golden archive with its
meta, the image / truth / loss cases as the wrappers take them, synthetic batches and a folder of frames with labels."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = 416
MAX_BOXES = 90


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "yolo_train.npz"))
    out = {k: g[k] for k in g.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def meta():
    return json.loads(bytes(golden()["meta"]).decode())


def image_case(c):
    """the arguments of yolo_inputs for image case ``c`` of the meta, and the reference's result [1, 3, net_h, net_w]"""
    g = golden()
    frames = np.array(g["frame%d" % c["frame"]])[None]
    hsv = None if c["hsv"] is None else np.array([c["hsv"]], np.float32)
    args = (frames, np.zeros(1, np.int32), np.array([c["crop"]], np.int32), np.array([c["flip"]], np.uint8), hsv, tuple(c["net"]))
    return args, np.array(g["img_" + c["name"]])[None]


def truth_case(c):
    """the arguments of yolo_truth for truth case ``c`` (one sample), and the reference's truth [1, 90, 5]"""
    g = golden()
    labels = np.array(g["truth_%s_labels" % c["name"]]).reshape(-1, 5)
    args = (labels, np.array([0, len(labels)], np.int32), np.array(g["truth_%s_swap" % c["name"]]),
            np.array([c["geom"]], np.float32), np.array([c["flip"]], np.uint8), c["classes"], MAX_BOXES, (NET, NET))
    return args, np.array(g["truth_%s_out" % c["name"]])[None]


def truth_batch():
    """every truth case with two classes as ONE batch (classes = 3 accepts all their ids): the arguments of yolo_truth"""
    g = golden()
    cs = meta()["truth_cases"]
    labels = [np.array(g["truth_%s_labels" % c["name"]]).reshape(-1, 5) for c in cs]
    swaps = [np.array(g["truth_%s_swap" % c["name"]]) for c in cs]
    first = np.concatenate([[0], np.cumsum([len(a) for a in labels])]).astype(np.int32)
    return (np.concatenate(labels), first, np.concatenate(swaps).astype(np.int32), np.array([c["geom"] for c in cs], np.float32),
            np.array([c["flip"] for c in cs], np.uint8), 3, MAX_BOXES, (NET, NET))


def loss_case(c):
    """(x, truth, kwargs of yolo_loss) for loss case ``c``, and the reference's (delta, act)"""
    g = golden()
    n = "loss_%s_" % c["name"]
    kw = dict(net_size=(NET, NET), anchors=np.array(g["anchors"]), mask=np.array(c["mask"], np.int32), classes=c["classes"],
              ignore_thresh=c["ignore_thresh"], truth_thresh=c["truth_thresh"])
    return np.array(g[n + "x"]), np.array(g[n + "truth"]), kw, np.array(g[n + "delta"]), np.array(g[n + "act"])


def line_values(line):
    """the seven numbers of the reference's ``Region ... Avg IOU: ...`` line: six floats and the count"""
    import re
    v = re.findall(r":\s*(-?nan|-?[0-9.]+)", line)
    assert len(v) == 7, line
    return [float(s) for s in v[:6]], int(v[6])


def frames_of(H, W, n=2, seed=5):
    """n uint8 RGB frames with a black block, a white block and a grey block in the first"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    f[0, :H // 4, :W // 4] = 0
    f[0, H // 4:H // 2, :W // 4] = 255
    f[0, H // 2:, :W // 4] = 77
    return f


def mixed_batch(H, W):
    """(frame_index, crop, flip, hsv) for B = 3 samples of an H x W frame pair: an inside crop distorted, one past every
    edge flipped, one narrow crop flipped and distorted with the hue wrapping the other way"""
    idx = np.array([0, 1, 0], np.int32)
    crop = np.array([(W // 9, H // 7, W - W // 4, H - H // 3), (-(W // 6), -(H // 5), W + W // 3, H + H // 2),
                     (W // 3, H // 8, 2 + W // 5, H - H // 4)], np.int32)
    flip = np.array([0, 1, 1], np.uint8)
    hsv = np.array([(0.09, 1.4, 0.8), (0.0, 1.0, 1.0), (-0.21, 0.7, 1.3)], np.float32)
    return idx, crop, flip, hsv


def synthetic_loss(w, h, classes, mask, B=2, seed=3, truths=6):
    """(x, truth) for a w x h grid: ``truths`` boxes sized about the anchors in image 0 (two in one cell), none in the last"""
    rng = np.random.default_rng([seed, w, h, classes])
    anchors = np.array(golden()["anchors"])
    x = rng.normal(0, 1.5, (B, len(mask) * (5 + classes), h, w)).astype(np.float32)
    t = np.zeros((B, MAX_BOXES, 5), np.float32)
    for b in range(B - 1):
        for k in range(truths):
            a = anchors[rng.integers(0, 9)] / NET * rng.uniform(0.8, 1.2, 2)
            cx, cy = (rng.uniform(0.02, 0.98, 2) if k else (0.51, 0.52))
            if k == 1:
                cx, cy = t[b, 0, 0], t[b, 0, 1]
            t[b, k] = (cx, cy, a[0], a[1], rng.integers(0, classes))
    return x, t


def write_folder(base, n=3, H=48, W=64, seed=11):
    """A synthetic Darknet data set: n PNG frames under base/JPEGImages, their label files under base/labels and the
    list file, whose path is returned."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(base, "JPEGImages"), exist_ok=True)
    os.makedirs(os.path.join(base, "labels"), exist_ok=True)
    paths = []
    for i in range(n):
        p = os.path.join(base, "JPEGImages", "%06d.png" % i)
        Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(p)
        with open(os.path.join(base, "labels", "%06d.txt" % i), "w") as f:
            for _ in range(i + 1):
                f.write("0 %.6f %.6f %.6f %.6f\n" % tuple(rng.uniform((0.3, 0.3, 0.1, 0.1), (0.7, 0.7, 0.4, 0.4))))
        paths.append(p)
    lst = os.path.join(base, "all.txt")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    return lst
