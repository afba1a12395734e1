"""Training batches and the criterion of the detector: Darknet's detection data path (``train_YOLO/src/data.c``
load_data_detection without OpenCV, fill_truth_detection, correct_boxes; ``image.c`` crop_image, resize_image,
flip_image, distort_image) and the training half of its ``[yolo]`` layer (``yolo_layer.c`` forward_yolo_layer).

The wrappers follow train_data.py: ``device=None`` runs the host twin of libbetapose_hip.so on numpy arrays (no GPU
needed), a torch device the kernels of csrc/yolo_train.hip on tensors that stay on that device; the two agree bit for
bit.  Definitions and declared deviations: DESIGN.md 3.11.  The network's backward pass is autograd's; an optimiser
loop, Darknet's learning-rate schedule, ``focal_loss`` and ``l.map`` are out of scope.
"""
from __future__ import annotations

import os

import numpy as np

from .train_data import _np, save_npz  # noqa: F401  (save_npz is part of this module's surface)

STAT_NAMES = ("iou", "class", "obj", "anyobj", "recall50", "recall75", "count")
# ------------------------------------------------------------------------------------------------ inputs
def yolo_inputs(frames, frame_index, crop, flip, hsv=None, net_size=(416, 416), device=None, out=None):
    """One sample of load_data_detection per row, without its random draws: ``out`` [B, 3, net_h, net_w] float32, a numpy
    array with ``device=None`` and a tensor on ``device`` otherwise.  ``frames`` [N, H, W, 3] uint8 **RGB** (an array,
    or a tensor already on the device), ``frame_index`` [B] (an index outside [0, N) gives a zero sample), ``crop``
    [B, 4] int32 = (pleft, ptop, swidth, sheight), ``flip`` [B], ``hsv`` [B, 3] float32 = (dhue, dsat, dexp) or None
    for no distortion, ``net_size`` = (net_h, net_w).  ``out`` may name the tensor (device) to write."""
    from . import _lib
    idx = _np(frame_index, np.int32).reshape(-1)
    B = len(idx)
    crop = _np(crop, np.int32).reshape(-1, 4)
    flip = _np(flip, np.uint8).reshape(-1)
    hsv = None if hsv is None else _np(hsv, np.float32).reshape(-1, 3)
    if len(crop) != B or len(flip) != B or (hsv is not None and len(hsv) != B):
        raise ValueError("crop, flip and hsv need one row per sample")
    if frames.ndim != 4 or frames.shape[3] != 3 or (frames.dtype != np.uint8 and str(frames.dtype) != "torch.uint8"):
        raise ValueError("frames must be uint8 [N, H, W, 3]")
    N, H, W = (int(v) for v in frames.shape[:3])
    net_h, net_w = int(net_size[0]), int(net_size[1])
    side = _lib.Side(device)
    res = side.empty((B, 3, net_h, net_w), np.float32) if device is None or out is None else out
    if res is out and (tuple(res.shape) != (B, 3, net_h, net_w) or res.dtype != side.torch.float32):
        raise ValueError("out must be float32 [B, 3, net_h, net_w]")
    side.call("bp_yolo_inputs", side.put(frames, np.uint8), N, H, W, side.put(idx), side.put(crop), side.put(flip), side.put(hsv),
              B, net_h, net_w, res)
    return res


# ------------------------------------------------------------------------------------------------ truth rows
def yolo_truth(labels, first, swap, geom, flip, classes=1, max_boxes=90, net_size=(416, 416), small_object=0, device=None):
    """fill_truth_detection with correct_boxes for ``B`` samples: ``(truth [B, max_boxes, 5], kept [B])``.  ``labels``
    [M, 5] float32 = (id, x, y, w, h) as read_labels returns them, ``first`` [B + 1] each sample's slice of them,
    ``swap`` [M] the index randomize_boxes draws at each step (within the sample's slice: ``random_gen() % n``), ``geom``
    [B, 4] float32 = (dx, dy, sx, sy) as load_data_detection passes them, ``flip`` [B].  A truth row is (x, y, w, h,
    id); the rows past ``kept[b]`` are zero.  The list is cut to ``max_boxes`` before the filter, as in the reference."""
    from . import _lib
    labels = _np(labels, np.float32).reshape(-1, 5)
    M = len(labels)
    first = _np(first, np.int32).reshape(-1)
    B = len(first) - 1
    swap = _np(swap, np.int32).reshape(-1)
    geom = _np(geom, np.float32).reshape(-1, 4)
    flip = _np(flip, np.uint8).reshape(-1)
    if B < 1 or len(swap) != M or len(geom) != B or len(flip) != B:
        raise ValueError("first needs B + 1 entries, swap one per label, geom and flip one row per sample")
    net_h, net_w = int(net_size[0]), int(net_size[1])
    if device is not None and (first[0] < 0 or first[-1] > M or (np.diff(first) < 0).any()):
        raise ValueError("first must be non-decreasing within [0, M]")
    side = _lib.Side(device)
    pad = lambda a, shape: a if M else np.zeros(shape, a.dtype)   # (an empty tensor has no address)
    order = side.empty(max(M, 1), np.int32)
    truth, kept = side.empty((B, max_boxes, 5), np.float32), side.empty(B, np.int32)
    side.call("bp_yolo_truth", side.put(pad(labels, (1, 5))), M, side.put(first), side.put(pad(swap, (1,))), side.put(geom),
              side.put(flip), B, classes, max_boxes, net_w, net_h, small_object, order, truth, kept)
    return truth, kept


# ------------------------------------------------------------------------------------------------ loss
def _loss_shapes(x, truth, mask, anchors, classes):
    if x.ndim != 4 or truth.ndim != 3 or truth.shape[2] != 5 or int(truth.shape[0]) != int(x.shape[0]):
        raise ValueError("x must be [B, C, h, w] and truth [B, max_boxes, 5]")
    B, C, h, w = (int(v) for v in x.shape)
    return B, C, h, w, int(truth.shape[1]), len(mask), len(anchors)


def _loss_call(side, x, truth, net_size, anchors, mask, classes, ignore_thresh, truth_thresh, focal_loss, want_act):
    """bp_yolo_loss on ``side``: a dict of its buffers (``cost`` [1], ``stats`` [7] float64)."""
    from . import _lib
    anchors = _np(anchors, np.float32).reshape(-1, 2)
    mask = _np(mask, np.int32).reshape(-1)
    B, C, h, w, max_boxes, n, total = _loss_shapes(x, truth, mask, anchors, classes)
    d_x, d_t = side.put(x, np.float32), side.put(truth, np.float32)
    shape = tuple(d_x.shape)
    r = {"cost": side.empty(1, np.float64), "stats": side.empty(7, np.float64), "delta": side.empty(shape, np.float32),
         "act": side.empty(shape, np.float32) if want_act else None}
    partial = side.empty(max(int(_lib.lib().bp_yolo_loss_partials(B, n, classes, h, w)), 1), np.float64)
    side.call("bp_yolo_loss", d_x, B, C, n, classes, h, w, int(net_size[1]), int(net_size[0]), side.put(anchors), total,
              side.put(mask), d_t, max_boxes, ignore_thresh, truth_thresh, int(focal_loss), r["act"], r["delta"], r["cost"],
              r["stats"], partial)
    return r


def yolo_loss(x, truth, net_size, anchors, mask, classes=1, ignore_thresh=0.7, truth_thresh=1.0, focal_loss=0, want_act=True,
              device=None):
    """forward_yolo_layer with ``train = 1`` for one head, ``(cost, stats, delta, act)``: ``x`` [B, n * (5 + classes), h, w]
    the raw head output, ``truth`` [B, max_boxes, 5] as yolo_truth makes it, ``net_size`` = (net_h, net_w), ``anchors``
    [total, 2] in pixels of the network input, ``mask`` [n] this head's anchors.  ``cost`` (float) the sum of delta^2
    in float64 in a fixed order (Darknet's float32 running sum is not reproduced); ``stats`` a dict of the float64 sums
    the reference's log line divides (STAT_NAMES); ``delta`` = l.delta and ``act`` = l.output, shaped as ``x`` (tensors
    on ``device``, arrays otherwise; ``act`` None without ``want_act``).  ``delta`` is the descent direction Darknet
    adds in backward_yolo_layer, not a derivative."""
    from . import _lib
    side = _lib.Side(device)
    r = _loss_call(side, x, truth, net_size, anchors, mask, classes, ignore_thresh, truth_thresh, focal_loss, want_act)
    return float(side.get(r["cost"])[0]), dict(zip(STAT_NAMES, side.get(r["stats"]).tolist())), r["delta"], r["act"]


def region_line(stats, cells, index=0):
    """The reference's log line of one head from ``stats``; ``cells`` = w * h * n * B."""
    c = stats["count"]
    div = lambda a: a / c if c else float("nan")
    return ("Region %d Avg IOU: %f, Class: %f, Obj: %f, No Obj: %f, .5R: %f, .75R: %f,  count: %d"
            % (index, div(stats["iou"]), div(stats["class"]), div(stats["obj"]), stats["anyobj"] / cells, div(stats["recall50"]),
               div(stats["recall75"]), int(c)))


def _yolo_loss_class():
    import torch

    class YoloLoss(torch.autograd.Function):
        """``YoloLoss.apply(x, truth, net_size, anchors, mask, classes, ignore_thresh, truth_thresh)`` -> the cost of one
        head as a float32 scalar tensor on ``x``'s device (a CPU tensor runs the host twin).  ``backward`` hands
        ``-delta * grad_output`` to ``x``.  This is Darknet's convention: ``delta`` is the descent direction that
        backward_yolo_layer adds to the network's delta, so its negative takes the place of a gradient.  It is NOT the
        analytic derivative of the cost ``sum(delta^2)``.  After a forward, ``YoloLoss.last`` holds that call's
        ``stats`` and ``delta``."""
        last = None

        @staticmethod
        def forward(ctx, x, truth, net_size, anchors, mask, classes=1, ignore_thresh=0.7, truth_thresh=1.0):
            if x.is_cuda:
                from . import _lib
                r = _loss_call(_lib.Side(x.device), x.detach(), truth.detach(), net_size, anchors, mask, classes, ignore_thresh,
                               truth_thresh, 0, False)
                cost, delta, stats = r["cost"][0].to(torch.float32), r["delta"], r["stats"]
            else:
                c, st, d, _ = yolo_loss(x.detach(), truth.detach(), net_size, anchors, mask, classes, ignore_thresh, truth_thresh,
                                        want_act=False)
                cost, delta, stats = torch.tensor(c, dtype=torch.float32), torch.from_numpy(d), st
            ctx.save_for_backward(delta)
            YoloLoss.last = {"stats": stats, "delta": delta}
            return cost

        @staticmethod
        def backward(ctx, grad_output):
            (delta,) = ctx.saved_tensors
            return (-delta * grad_output.to(delta.dtype),) + (None,) * 7

    return YoloLoss


def __getattr__(name):     # YoloLoss is built on first use, so importing this module does not import torch
    if name == "YoloLoss":
        cls = _yolo_loss_class()
        globals()["YoloLoss"] = cls
        return cls
    raise AttributeError(name)


def yolo_head_params(cfg_blocks):
    """The ``[yolo]`` blocks of a parsed cfg (cfg.parse_cfg), in order: a list of dicts of ``mask`` [n] int32,
    ``anchors`` [total, 2] float32, ``classes``, ``ignore_thresh`` and ``truth_thresh`` (parser.c's defaults .5 and 1)."""
    heads = []
    for b in cfg_blocks:
        if b.get("type") != "yolo":
            continue
        a = np.array([float(v) for v in b["anchors"].split(",")], np.float32).reshape(-1, 2)
        total = int(b.get("num", len(a)))
        if len(a) < total:
            raise ValueError("a [yolo] block names %d anchors and lists %d" % (total, len(a)))
        mask = (np.array([int(v) for v in b["mask"].split(",")], np.int32) if "mask" in b else np.arange(total, dtype=np.int32))
        heads.append(dict(mask=mask, anchors=a[:total].copy(), classes=int(b.get("classes", 20)),
                          ignore_thresh=float(b.get("ignore_thresh", .5)), truth_thresh=float(b.get("truth_thresh", 1))))
    return heads


# ------------------------------------------------------------------------------------------------ draws, labels
def _uniform(rng, lo, hi, B):
    """rand_uniform_strong in float32: ``random_float() * (max - min) + min``."""
    lo, hi = np.float32(min(lo, hi)), np.float32(max(lo, hi))
    return (rng.random(B, dtype=np.float32) * (hi - lo) + lo).astype(np.float32)


def _scale(rng, s, B):
    """rand_scale: ``U(1, s)``, or its reciprocal (a double division stored as float) with probability 1 / 2."""
    v = _uniform(rng, 1, s, B)
    keep = rng.integers(0, 2, B).astype(bool)
    return np.where(keep, v, (1.0 / v.astype(np.float64)).astype(np.float32)).astype(np.float32)


def draw_detection_augmentation(rng, B, image_size, jitter=0.3, hue=0.3, saturation=1.5, exposure=1.5, flip=True):
    """load_data_detection's per-sample draws for ``B`` frames of ``image_size`` = (oh, ow) from ``rng``
    (``numpy.random.default_rng(seed)``): ``(crop [B, 4] int32, geom [B, 4] float32, flip [B] uint8, hsv [B, 3]
    float32)``.  The distributions are the reference's -- ``dw = (int)(ow * jitter)``, the four margins
    ``(int) rand_uniform_strong(-dw, dw)`` truncated toward zero, ``sx = swidth / ow``, ``dx = (pleft / ow) / sx`` and
    ``geom`` = (dx, dy, 1 / sx, 1 / sy) in float32 with the reciprocal formed in double, ``dhue = U(-hue, hue)``,
    ``dsat``, ``dexp`` = rand_scale -- but the numbers come from a numpy generator: they do NOT reproduce ``rand()``'s
    bits, nor the order in which the reference interleaves its draws.  A crop narrower than two pixels is drawn again."""
    oh, ow = int(image_size[0]), int(image_size[1])
    dw, dh = int(np.float32(ow) * np.float32(jitter)), int(np.float32(oh) * np.float32(jitter))
    crop = np.empty((B, 4), np.int32)
    for b in range(B):
        while True:
            pl, pr = (int(v) for v in _uniform(rng, -dw, dw, 2))
            pt, pb = (int(v) for v in _uniform(rng, -dh, dh, 2))
            if ow - pl - pr >= 2 and oh - pt - pb >= 2:
                break
        crop[b] = (pl, pt, ow - pl - pr, oh - pt - pb)
    f32 = np.float32
    sx, sy = crop[:, 2].astype(f32) / f32(ow), crop[:, 3].astype(f32) / f32(oh)
    dx, dy = (crop[:, 0].astype(f32) / f32(ow)) / sx, (crop[:, 1].astype(f32) / f32(oh)) / sy
    geom = np.stack([dx, dy, (1.0 / sx.astype(np.float64)).astype(f32), (1.0 / sy.astype(np.float64)).astype(f32)], 1)
    fl = rng.integers(0, 2, B).astype(np.uint8) if flip else np.zeros(B, np.uint8)
    hsv = np.stack([_uniform(rng, -hue, hue, B), _scale(rng, saturation, B), _scale(rng, exposure, B)], 1).astype(f32)
    return crop, np.ascontiguousarray(geom, f32), fl, hsv


def identity_augmentation(B, image_size):
    """The draws of an undistorted, unflipped, uncropped sample (evaluation mode): hsv is None."""
    oh, ow = int(image_size[0]), int(image_size[1])
    crop = np.tile(np.array([0, 0, ow, oh], np.int32), (B, 1))
    geom = np.tile(np.array([0, 0, 1, 1], np.float32), (B, 1))
    return crop, geom, np.zeros(B, np.uint8), None


_LABEL_DIRS = (("/images/train2014/", "/labels/train2014/"), ("/images/val2014/", "/labels/val2014/"), ("/JPEGImages/", "/labels/"),
               ("\\images\\train2014\\", "\\labels\\train2014\\"), ("\\images\\val2014\\", "\\labels\\val2014\\"),
               ("\\JPEGImages\\", "\\labels\\"))
_LABEL_EXTS = (".jpg", ".JPG", ".jpeg", ".JPEG", ".png", ".PNG", ".bmp", ".BMP", ".ppm", ".PPM")


def label_path(image_path):
    """replace_image_to_label: the first occurrence of each image directory becomes its label directory, blanks and tabs
    are trimmed, and an image extension becomes ``.txt`` where its first occurrence in the path is the path's end."""
    p = image_path
    for a, b in _LABEL_DIRS:
        p = p.replace(a, b, 1)
    p = p.strip(" \t")
    for e in _LABEL_EXTS:
        i = p.find(e)
        if i >= 0 and i + len(e) == len(p):
            p = p[:i] + ".txt"
    return p


def read_labels(paths):
    """read_boxes over the label files ``paths``: ``(labels [M, 5] float32 = (id, x, y, w, h), first [B + 1] int32)``.
    As fscanf does, reading stops at the first token that does not parse; a missing file holds no box."""
    rows, first = [], [0]
    for p in paths:
        if os.path.exists(p):
            tok = open(p).read().split()
            for i in range(0, len(tok) - 4, 5):
                try:
                    rows.append((int(tok[i]),) + tuple(float(v) for v in tok[i + 1:i + 5]))
                except ValueError:
                    break
        first.append(len(rows))
    return np.array(rows, np.float32).reshape(-1, 5), np.array(first, np.int32)


def draw_swaps(rng, first):
    """randomize_boxes' draws: for each label an index within its sample's slice."""
    n = np.diff(first)
    return np.concatenate([rng.integers(0, k, k) for k in n if k] + [np.zeros(0, np.int64)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ loader
class YoloSampleLoader:
    """Iterate ``(inps [b, 3, net_h, net_w], truth [b, max_boxes, 5])`` over the images ``list_file`` names (one path per
    line, Darknet's ``train=`` list; the labels lie where label_path says), ``batch`` samples at a time (the last batch
    may be smaller).  The frames are decoded ahead by FrameLoader (BGR, reversed to RGB here) and must share one size.
    ``train`` shuffles the list with ``seed`` and draws the augmentation (``**augmentation``: the keywords of
    draw_detection_augmentation); the evaluation mode takes the list in order, whole frames, undistorted.  With a
    ``device`` both results are tensors on it, else numpy arrays from the host twins; the same seed gives the same bits
    either way.  ``last`` holds the draws of the batch just yielded."""

    def __init__(self, list_file, batch, net_size=(416, 416), classes=1, max_boxes=90, seed=0, train=True, device=None,
                 threads=8, depth=16, **augmentation):
        with open(list_file) as f:
            self.paths = [ln.strip() for ln in f if ln.strip()]
        self.batch, self.net_size, self.classes, self.max_boxes = int(batch), tuple(net_size), int(classes), int(max_boxes)
        if self.batch < 1:
            raise ValueError("batch must be positive")
        self.seed, self.train, self.device, self.augmentation = int(seed), bool(train), device, dict(augmentation)
        self.threads, self.depth = threads, max(int(depth), 2)
        self.epoch = 0
        self.last = None

    def __len__(self):
        return (len(self.paths) + self.batch - 1) // self.batch

    def _batch(self, rng, ids, frames):
        B, (H, W) = len(ids), frames.shape[1:3]
        if self.train:
            crop, geom, flip, hsv = draw_detection_augmentation(rng, B, (H, W), **self.augmentation)
        else:
            crop, geom, flip, hsv = identity_augmentation(B, (H, W))
        labels, first = read_labels([label_path(self.paths[i]) for i in ids])
        swap = draw_swaps(rng, first)
        dev = self.device
        inps = yolo_inputs(frames, np.arange(B, dtype=np.int32), crop, flip, hsv, self.net_size, dev)
        truth, kept = yolo_truth(labels, first, swap, geom, flip, self.classes, self.max_boxes, self.net_size, 0, dev)
        self.last = dict(ids=np.asarray(ids), crop=crop, geom=geom, flip=flip, hsv=hsv, labels=labels, first=first, swap=swap,
                         kept=kept)
        return inps, truth

    def __iter__(self):
        from .frame_loader import FrameLoader
        N = len(self.paths)
        rng = np.random.default_rng([self.seed, self.epoch])
        self.epoch += 1
        order = rng.permutation(N) if self.train else np.arange(N)
        if N == 0:
            return
        loader = FrameLoader([self.paths[i] for i in order], threads=self.threads, depth=self.depth, pinned=False)
        try:
            held = []
            for k, frame, _ in loader:
                held.append(np.ascontiguousarray(frame[..., ::-1]))     # BGR -> RGB, copied out of the slot
                loader.release(k)
                if len(held) == self.batch or k == N - 1:
                    ids = order[k + 1 - len(held):k + 1]
                    yield self._batch(rng, ids, np.stack(held))
                    held = []
        finally:
            loader.close()
