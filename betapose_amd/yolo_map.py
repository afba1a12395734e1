"""Detector validation: Darknet's ``./darknet detector map`` (``train_YOLO/src/detector.c`` validate_detector_map) --
the box list of get_network_boxes + do_nms_sort, the matching against the label files and the 11-point AP, mAP,
precision, recall, F1 and average IoU it prints.

The wrappers follow yolo_train.py: ``device=None`` runs the host twins of libbetapose_hip.so on numpy arrays (no GPU
needed), a torch device the kernels of csrc/yolo_map.hip on tensors that stay on that device; the two agree bit for bit.
Definitions and declared deviations: DESIGN.md 3.12.  ``detector recall``, letterbox input, ``difficult=`` and ``map=``
are out of scope.
"""
from __future__ import annotations

import numpy as np

from .train_data import _np

STAT_NAMES = ("mAP", "precision", "recall", "f1", "avg_iou", "tp", "fp", "fn")
REC = 6     # words of a record: p, image, class, truth, max_iou, position within the image
def heads_table(shapes):
    """The head table of yolo_detections from ``shapes`` = [(anchors, gh, gw), ...] in the order of the cfg's ``[yolo]``
    blocks: int32 [nheads, 4] = (first row, anchors, gh, gw)."""
    rows, at = [], 0
    for n, gh, gw in shapes:
        rows.append((at, int(n), int(gh), int(gw)))
        at += int(n) * int(gh) * int(gw)
    return np.array(rows, np.int32).reshape(-1, 4)


def cfg_heads(blocks):
    """``(net_h, net_w, [(anchors, gh, gw), ...], classes)`` of a parsed cfg (cfg.parse_cfg): the ``[yolo]`` blocks in order,
    each with the grid its input has.  The grid follows the layers' strides: convolutional and maxpool divide (rounding
    up, as ``pad=1`` does), upsample multiplies, route takes its first layer's, shortcut and yolo keep it."""
    net = blocks[0] if blocks and blocks[0].get("type") == "net" else {}
    h, w = int(net.get("height", 416)), int(net.get("width", 416))
    sizes, shapes, classes = [], [], None
    for b in (b for b in blocks if b.get("type") != "net"):
        t = b["type"]
        if t in ("convolutional", "maxpool"):
            s = int(b.get("stride", 1))
            h, w = (h + s - 1) // s, (w + s - 1) // s
        elif t == "upsample":
            h, w = h * int(b.get("stride", 2)), w * int(b.get("stride", 2))
        elif t == "route":
            i = int(str(b["layers"]).split(",")[0])
            h, w = sizes[i if i >= 0 else len(sizes) + i]
        elif t == "yolo":
            n = len(str(b["mask"]).split(",")) if "mask" in b else int(b.get("num", 1))
            if classes not in (None, int(b.get("classes", 20))):
                raise ValueError("the [yolo] blocks differ in classes")
            classes = int(b.get("classes", 20))
            shapes.append((n, h, w))
        sizes.append((h, w))
    if not shapes:
        raise ValueError("the cfg holds no [yolo] block")
    net_h, net_w = int(net.get("height", 416)), int(net.get("width", 416))
    return net_h, net_w, shapes, classes


def max_dets_cap():
    from . import _lib
    return int(_lib.lib().bp_yolo_map_max_dets())


def _detections(side, pred, heads, net_size, classes, thresh, nms, max_dets):
    from . import _lib
    B, rows, attrs = (int(v) for v in pred.shape)
    dets, count = side.empty((B, max_dets, 6 + classes), np.float32), side.empty(B, np.int32)
    scratch = [] if side.dev is None else [side.empty(max(int(_lib.lib().bp_yolo_detections_scratch(B, max_dets, classes)), 4) // 4)]
    side.call("bp_yolo_detections", side.put(pred, np.float32), B, rows, attrs, _lib.ptr(heads), len(heads), int(net_size[1]),
              int(net_size[0]), classes, thresh, nms, max_dets, dets, count, *scratch)
    return dets, count


def yolo_detections(pred, heads, net_size, classes, thresh=.005, nms=.45, max_dets=1024, device=None):
    """Darknet's box list for a batch: ``get_network_boxes(net, 1, 1, thresh, 0, 0, 0, &n, 0)`` then ``do_nms_sort(dets, n,
    classes, nms)`` per image.  ``pred`` [B, rows, 5 + classes] float32 as bp_yolo_forward writes it (boxes in detector-input
    pixels), ``heads`` = heads_table(...), ``net_size`` = (net_h, net_w).  Returns ``(dets [B, max_dets, 6 + classes],
    count [B], overflow)``: a row is (x, y, w, h, objectness, candidate index as int bits, prob[classes]) in the order the
    last class's sort left, zero past the count; ``count`` is the true number of candidates.  An image with more than
    ``max_dets`` (at most max_dets_cap() on a device) has a zero block and is done again by the host twin without a cap:
    ``overflow`` maps its index to its rows [count, 6 + classes] (a numpy array).  With ``device=None`` everything is
    numpy, else ``dets`` and ``count`` are tensors on ``device``."""
    from . import _lib
    heads = np.ascontiguousarray(heads, np.int32).reshape(-1, 4)
    if pred.ndim != 3 or int(pred.shape[2]) != 5 + classes:
        raise ValueError("pred must be [B, rows, 5 + classes]")
    rows = int(pred.shape[1])
    side = _lib.Side(device)
    dets, count = _detections(side, pred, heads, net_size, classes, thresh, nms, max_dets)
    overflow = {}
    for b in np.nonzero(side.get(count) > max_dets)[0]:
        d, c1 = _detections(_lib.Side(), pred[int(b):int(b) + 1], heads, net_size, classes, thresh, nms, rows)
        overflow[int(b)] = d[0, :int(c1[0])].copy()
    return dets, count, overflow


def map_match(dets, count, labels, first, classes, iou_thresh=.5, thresh_calc=.25, truth_base=0, image_base=0, rec_stride=None,
              truth_classes_count=None, device=None):
    """detector.c:665-756 for a batch: ``dets``, ``count`` from yolo_detections, ``labels`` [M, 5] = (id, x, y, w, h) and
    ``first`` [B + 1] as read_labels returns them.  Returns a dict of ``rec`` [B, rec_stride, 6] float32 (p, image, class,
    truth, max_iou, position; ints as bits; truth = ``truth_base`` + the label's index, or -1), ``rec_count`` [B],
    ``truth_classes_count`` [classes] int32 (the one passed in, added to) and ``img_stats`` [B, 3] float64 = (tp, fp,
    iou_sum) at ``thresh_calc``.  ``rec_stride`` defaults to what the largest image needs."""
    from . import _lib
    labels = _np(labels, np.float32).reshape(-1, 5)
    first = _np(first, np.int32).reshape(-1)
    M, B, max_dets = len(labels), len(first) - 1, int(dets.shape[1])
    if dets.ndim != 3 or int(dets.shape[0]) != B or int(dets.shape[2]) != 6 + classes:
        raise ValueError("dets must be [B, max_dets, 6 + classes] and first hold B + 1 entries")
    if first[0] < 0 or first[-1] > M or (np.diff(first) < 0).any():
        raise ValueError("first must be non-decreasing within [0, M]")
    side = _lib.Side(device)
    d, c = side.put(dets, np.float32), side.put(count, np.int32)
    if rec_stride is None:
        ch = side.get(c)
        rec_stride = max(int(np.where(ch > max_dets, 0, ch).max(initial=0)) * classes, 1)
    tcc = side.zeros(classes, np.int32) if truth_classes_count is None else truth_classes_count
    r = dict(rec=side.empty((B, rec_stride, REC), np.float32), rec_count=side.empty(B, np.int32), truth_classes_count=tcc,
             img_stats=side.empty((B, 3), np.float64))
    claim = [] if side.dev is None else [side.empty(M + 1, np.int32)]
    side.call("bp_detector_map_match", d, c, B, max_dets, classes, side.put(labels if M else np.zeros((1, 5), np.float32)), M,
              side.put(first), iou_thresh, thresh_calc, truth_base, image_base, rec_stride, r["rec"], r["rec_count"], tcc,
              r["img_stats"], *claim)
    return r


def map_reduce(rec, truth_classes_count, truths, img_stats, classes, want_pr=False, device=None):
    """detector.c:774-876 over the run's records ``rec`` [D, 6]: a dict of ``ap`` [classes] float64, ``stats`` [8] float64
    (STAT_NAMES) and ``pr`` [classes, D, 2] = (precision, recall) per rank, or None.  ``truths`` = unique_truth_count,
    ``img_stats`` [N, 3] the images' (tp, fp, iou_sum) in index order."""
    from . import _lib
    D, N = int(rec.shape[0]), int(img_stats.shape[0])
    side = _lib.Side(device)
    r = dict(ap=side.empty(classes, np.float64), stats=side.empty(8, np.float64),
             pr=side.empty((classes, D, 2), np.float64) if want_pr else None)
    scratch = [] if side.dev is None else [side.empty(max(int(_lib.lib().bp_detector_map_reduce_scratch(D, int(truths))), 8) // 8 + 1,
                                                      np.int64)]
    side.call("bp_detector_map_reduce", side.put(rec, np.float32) if D else None, D, side.put(truth_classes_count, np.int32), classes,
              int(truths), side.put(img_stats, np.float64) if N else None, N, r["ap"], r["stats"], r["pr"] if D else None, *scratch)
    return r


class DetectorMap:
    """The running state of one ``detector map`` run: ``update(pred, labels, first)`` per batch, ``result()`` at the end.
    ``heads`` = heads_table(...), ``net_size`` = (net_h, net_w).  Images are numbered in the order of the ``update`` calls
    unless ``image_base`` names a batch's first index; the result does not depend on the order of the calls."""

    def __init__(self, classes, heads, net_size, iou_thresh=.5, thresh_calc=.25, thresh=.005, nms=.45, max_dets=1024, device=None):
        self.classes, self.heads, self.net_size = int(classes), np.ascontiguousarray(heads, np.int32).reshape(-1, 4), tuple(net_size)
        self.iou_thresh, self.thresh_calc, self.thresh, self.nms = float(iou_thresh), float(thresh_calc), float(thresh), float(nms)
        self.max_dets, self.device = int(max_dets), device
        self.images = self.truths = 0
        self.chunks = []            # (image_base, rec [D_b, 6], img_stats [B, 3])
        self.tcc = None
        self.overflow = []

    def _cat(self, parts, width, dtype):
        if self.device is None:
            return np.concatenate(parts) if parts else np.zeros((0, width), dtype)
        import torch
        if parts:
            return torch.cat(parts)
        return torch.zeros((0, width), dtype=getattr(torch, np.dtype(dtype).name), device=self.device)

    def update(self, pred, labels, first, image_base=None, truth_base=None):
        """One batch: ``pred`` [B, rows, 5 + classes], ``labels`` [M, 5] and ``first`` [B + 1] as read_labels gives them.
        ``image_base`` numbers the batch's first image and ``truth_base`` its first label (defaults: in the order of the
        calls); a list that is walked in another order names both, and gives the same result."""
        classes, dev = self.classes, self.device
        tb = self.truths if truth_base is None else int(truth_base)
        labels = _np(labels, np.float32).reshape(-1, 5)
        first = _np(first, np.int32).reshape(-1)
        B = len(first) - 1
        base = self.images if image_base is None else int(image_base)
        dets, count, over = yolo_detections(pred, self.heads, self.net_size, classes, self.thresh, self.nms, self.max_dets, dev)
        r = map_match(dets, count, labels, first, classes, self.iou_thresh, self.thresh_calc, tb, base, None, self.tcc, dev)
        self.tcc = r["truth_classes_count"]
        rec, rc, st = r["rec"], r["rec_count"], r["img_stats"]
        if dev is None:
            keep = np.arange(rec.shape[1])[None, :] < rc[:, None]
            parts = [rec[keep]]
        else:
            import torch
            keep = torch.arange(rec.shape[1], device=rec.device)[None, :] < rc[:, None]
            parts = [rec[keep]]
        for b, rows in over.items():        # the uncapped answer of the host twins for the images the cap cut
            f0, f1 = int(first[b]), int(first[b + 1])
            n = max(len(rows), 1)
            d1 = np.zeros((1, n, 6 + classes), np.float32)
            d1[0, :len(rows)] = rows
            h = map_match(d1, np.array([len(rows)], np.int32), labels[f0:f1], np.array([0, f1 - f0], np.int32), classes,
                          self.iou_thresh, self.thresh_calc, tb + f0, base + b)
            hr, hs = h["rec"][0, :int(h["rec_count"][0])], h["img_stats"]
            if dev is not None:
                hr, hs = torch.from_numpy(hr).to(rec.device), torch.from_numpy(hs).to(rec.device)
            parts.append(hr)
            st[b] = hs[0]
            self.overflow.append(base + b)
        self.chunks.append((base, self._cat(parts, REC, np.float32), st))
        self.images = max(self.images, base + B)
        self.truths += len(labels)
        return dets, count

    def result(self, want_pr=False):
        chunks = sorted(self.chunks, key=lambda c: c[0])
        rec = self._cat([c[1] for c in chunks], REC, np.float32)
        st = self._cat([c[2] for c in chunks], 3, np.float64)
        tcc = self.tcc if self.tcc is not None else np.zeros(self.classes, np.int32)
        r = map_reduce(rec, tcc, self.truths, st, self.classes, want_pr, self.device)
        ap, stats = (_np(r[k], np.float64) for k in ("ap", "stats"))
        out = dict(zip(STAT_NAMES, stats.tolist()))
        for k in ("tp", "fp", "fn"):
            out[k] = int(out[k])
        out.update(ap=ap, detections_count=int(rec.shape[0]), unique_truth_count=int(self.truths),
                   truth_classes_count=_np(tcc, np.int32).copy(), overflow_images=sorted(self.overflow), thresh_calc=self.thresh_calc,
                   pr=r["pr"])
        return out


# ------------------------------------------------------------------------------------------------ the .data file, the report
def read_data_cfg(path):
    """read_data_cfg: the ``key = value`` lines of a Darknet ``.data`` file as a dict of strings (``#`` and ``;`` start a
    comment line, blanks around keys and values are dropped).  ``classes`` is an int where present."""
    opts = {}
    with open(path) as f:
        for ln in f:
            ln = ln.strip()
            if not ln or ln[0] in "#;" or "=" not in ln:
                continue
            k, v = ln.split("=", 1)
            opts[k.strip()] = v.strip()
    if "classes" in opts:
        opts["classes"] = int(opts["classes"])
    return opts


def report_lines(result, names):
    """The lines validate_detector_map prints, from DetectorMap.result()."""
    t = result["thresh_calc"]
    lines = ["detections_count = %d, unique_truth_count = %d  " % (result["detections_count"], result["unique_truth_count"])]
    for i, ap in enumerate(result["ap"]):
        lines.append("class_id = %d, name = %s, \t ap = %2.2f %% " % (i, names[i] if i < len(names) else "", ap * 100))
    lines.append(" for thresh = %1.2f, precision = %1.2f, recall = %1.2f, F1-score = %1.2f "
                 % (t, result["precision"], result["recall"], result["f1"]))
    lines.append(" for thresh = %0.2f, TP = %d, FP = %d, FN = %d, average IoU = %2.2f %% "
                 % (t, result["tp"], result["fp"], result["fn"], result["avg_iou"] * 100))
    lines.append("")
    lines.append(" mean average precision (mAP) = %f, or %2.2f %% " % (result["mAP"], result["mAP"] * 100))
    return lines
