"""Training batches, criterion and metric of the key-point detector: everything around the network in the reference's
``train_KPD/src/train.py`` train() / valid() loop (``utils/pose.py`` generateSampleBox, ``utils/img.py`` cropBox / flip /
shuffleLR, ``torchsample``'s Rotate, ``MSELoss(out * setMask, labels)``, ``utils/eval.py`` heatmapAccuracy).

The wrappers follow annotate.py: ``device=None`` runs the host twin of libbetapose_hip.so on numpy arrays (no GPU
needed), a torch device the kernels of csrc/kpd_sample.hip on tensors that stay on that device; the two agree bit for
bit.  Definitions: DESIGN.md 3.10.  The random draws come from a ``numpy.random.Generator``: the reference's draws are
reproduced in distribution, not Python's ``random`` stream.
"""
from __future__ import annotations

import math
import os

import numpy as np

from . import _lib
from .annotate import kpd_targets, kpd_windows

MEAN_RGB = (0.406, 0.457, 0.480)
_np = _lib.Side().put       # (an array, a tensor or None, dtype) -> a contiguous numpy array


def _windows(ul, br, B):
    ul = _np(ul, np.float32).reshape(-1, 2)
    br = _np(br, np.float32).reshape(-1, 2)
    if len(ul) != B or len(br) != B:
        raise ValueError("ul and br need one row per sample")
    if not (np.isfinite(ul).all() and np.isfinite(br).all()):
        raise ValueError("the windows must be finite")
    return ul, br


def kpd_inputs(frames, frame_index, ul, br, gains=None, blank=None, in_res=(320, 256), device=None):
    """The image half of generateSampleBox for ``B`` samples: ``inp`` [B, 3, inpH, inpW] float32, a numpy array with
    ``device=None`` and a tensor on ``device`` otherwise.  ``frames`` [N, H, W, 3] uint8 **RGB** (an array, or a tensor
    already on the device), ``frame_index`` [B] the frame of each sample, ``ul``, ``br`` [B, 2] float32 the windows
    kpd_targets takes, ``gains`` [B, 3] float32 the colour gains (None: no multiply, the evaluation mode), ``blank`` [B]
    non-zero where the sample is zeroed (the reference's ``jointNum == 0``).  A tap of the frame is
    ``clamp(u8 / 255 * gain, 0, 1) - mean`` in float32 (the division by 255 always happens; the reference's
    im_to_torch skips it for an image whose maximum is 0 or 1); the window is cropBox's: corners truncated toward zero,
    padded with zeros to the input's aspect ratio about its centre (ceil before, floor after), resized bilinearly with
    ``align_corners=True``."""
    idx = np.ascontiguousarray(_np(frame_index, np.int32)).reshape(-1)
    B = len(idx)
    ul, br = _windows(ul, br, B)
    if frames.ndim != 4 or frames.shape[3] != 3 or (frames.dtype != np.uint8 and str(frames.dtype) != "torch.uint8"):
        raise ValueError("frames must be uint8 [N, H, W, 3]")
    N, H, W = (int(v) for v in frames.shape[:3])
    if B and (idx.min() < 0 or idx.max() >= N):
        raise ValueError("a frame index lies outside [0, %d)" % N)
    inpH, inpW = int(in_res[0]), int(in_res[1])
    if min(inpH, inpW) < 1:
        raise ValueError("the input resolution must be positive")
    gains = None if gains is None else _np(gains, np.float32).reshape(-1, 3)
    blank = None if blank is None else _np(blank, np.uint8).reshape(-1)
    if (gains is not None and len(gains) != B) or (blank is not None and len(blank) != B):
        raise ValueError("gains and blank need one row per sample")
    side = _lib.Side(device)
    inp = side.empty((B, 3, inpH, inpW), np.float32)
    if B:
        side.call("bp_kpd_inputs", side.put(frames, np.uint8), N, H, W, side.put(idx), side.put(ul), side.put(br), side.put(gains),
                  side.put(blank), B, inpH, inpW, inp)
    return inp


def channel_table(C, flip_pairs=()):
    """shuffleLR as a table: entry ``c`` is the channel a flipped sample's channel ``c`` is read from.  ``flip_pairs``
    holds 1-based pairs as ``dataset.flipRef`` does; they are applied in order, as the reference swaps them."""
    perm = list(range(int(C)))
    for a, b in flip_pairs:
        a, b = int(a) - 1, int(b) - 1
        if not (0 <= a < C and 0 <= b < C):
            raise ValueError("flip pair (%d, %d) lies outside 1 .. %d" % (a + 1, b + 1, C))
        perm[a], perm[b] = perm[b], perm[a]
    return np.asarray(perm, dtype=np.int32)


def rotation_terms(angle_deg):
    """``(cos, sin)`` [B, 2] float64 of ``pi / 180 * angle``, formed once here for both the host twin and the kernel
    (neither calls a trigonometric function); an angle of 0 gives exactly (1, 0), which both read as "no rotation"."""
    a = np.ascontiguousarray(angle_deg, dtype=np.float64).reshape(-1)
    if not np.isfinite(a).all():
        raise ValueError("angles must be finite")
    return np.ascontiguousarray([[1.0, 0.0] if v == 0.0 else [math.cos(math.pi / 180.0 * v), math.sin(math.pi / 180.0 * v)]
                                 for v in a], dtype=np.float64).reshape(-1, 2)


def augment_maps(x, flip, angle_deg, flip_pairs=(), device=None):
    """Flip, shuffleLR and Rotate of ``x`` [B, C, H, W] float32 in one pass (a new array / tensor, as kpd_inputs returns
    them).  ``flip`` [B] non-zero: column ``j`` takes column ``W - 1 - j`` (img.py flip) and the channels of
    ``flip_pairs`` (1-based pairs) are swapped.  ``angle_deg`` [B] float64: ``torchsample.transforms.Rotate(angle)`` of
    the flipped map, restated from its published source -- source coordinate ``A (dst - centre) + centre`` with
    ``A = [[cos, -sin], [sin, cos]]`` on (row, col) and centre ``(H/2 - 0.5, W/2 - 0.5)`` in float64, bilinear taps with
    the coordinate clamped to the map (edge replication), blended in float32.  A sample with ``flip = 0`` and
    ``angle = 0`` is copied."""
    if x.ndim != 4:
        raise ValueError("x must be [B, C, H, W]")
    B, C, H, W = (int(v) for v in x.shape)
    flip = _np(flip, np.uint8).reshape(-1)
    cs = rotation_terms(_np(angle_deg, np.float64))
    if len(flip) != B or len(cs) != B:
        raise ValueError("flip and angle_deg need one entry per sample")
    perm = channel_table(C, flip_pairs) if len(flip_pairs) else None
    side = _lib.Side(device)
    d_x = side.put(x, np.float32)
    y = side.empty(tuple(d_x.shape), np.float32)
    if B * C * H * W:
        side.call("bp_kpd_augment", d_x, B, C, H, W, side.put(flip), side.put(cs), side.put(perm), y)
    return y


def _loss_shapes(out, labels, set_mask):
    if out.ndim != 4 or tuple(labels.shape) != tuple(out.shape) or (set_mask is not None and tuple(set_mask.shape) != tuple(out.shape)):
        raise ValueError("out, labels and set_mask must share one shape [B, K, H, W]")
    B, K, H, W = (int(v) for v in out.shape)
    if min(B, K, H, W) < 1:
        raise ValueError("B, K, H and W must be positive")
    return B, K, H, W


def _loss_call(side, out, labels, set_mask, want_grad):
    """bp_heatmap_loss_acc on ``side``: a dict of its buffers (``loss`` [1] float64)."""
    B, K, H, W = _loss_shapes(out, labels, set_mask)
    d_out, d_lab, d_mask = (side.put(a, np.float32) for a in (out, labels, set_mask))
    r = {"loss": side.empty(1, np.float64), "acc": side.empty(K + 1, np.float32), "preds": side.empty((B, K, 2), np.int32),
         "gt": side.empty((B, K, 2), np.int32), "dists": side.empty((K, B), np.float32),
         "grad": side.empty((B, K, H, W), np.float32) if want_grad else None}
    partial = side.empty(B * K, np.float64)
    side.call("bp_heatmap_loss_acc", d_out, d_lab, d_mask, B, K, H, W, partial, r["loss"], r["acc"], r["preds"], r["gt"],
              r["dists"], r["grad"])
    return r


def heatmap_loss_accuracy(out, labels, set_mask=None, want_grad=False, device=None):
    """The reference's criterion and metric of one batch, ``(loss, acc, preds, gt, dists, grad)``:

    ``loss`` (float) the mean of ``(out * set_mask - labels)^2`` -- product and difference in float32 as the reference
    forms them, the squares summed in float64 in a fixed order, so the value has the same bits on every run;
    ``acc`` [K + 1] float32 heatmapAccuracy over every channel (``acc[1 + k]`` the share of channel ``k``'s counted
    samples within ``0.5 * H / 10`` px, -1 when none counts; ``acc[0]`` the mean of the non-negative ones, 0 when none);
    ``preds``, ``gt`` [B, K, 2] int32 getPreds of ``out * set_mask`` and of ``labels`` as (x, y), the lowest flat index
    among equal maxima; ``dists`` [K, B] float32 calc_dists with ``norm = H / 10``, -1 unless ``gt.x > 0 and gt.y > 0``;
    ``grad`` [B, K, H, W] float32 = ``((float32)(2 / N) * (out * mask - labels)) * mask`` with ``want_grad``, else None
    (a tensor on ``device``; everything else is returned on the host)."""
    _loss_shapes(out, labels, set_mask)
    side = _lib.Side(device)
    r = _loss_call(side, out, labels, set_mask, want_grad)
    return (float(side.get(r["loss"])[0]), side.get(r["acc"]), side.get(r["preds"]), side.get(r["gt"]), side.get(r["dists"]),
            r["grad"])


def _heatmap_mse_class():
    import torch

    class HeatmapMSE(torch.autograd.Function):
        """``HeatmapMSE.apply(out, labels, set_mask=None)`` -> the loss as a float32 scalar tensor on ``out``'s device,
        computed by bp_heatmap_loss_acc; ``backward`` hands ``grad * grad_output`` to ``out`` (labels and mask get no
        gradient).  After a forward, ``HeatmapMSE.last`` holds that call's ``acc``, ``preds``, ``gt`` and ``dists``
        as device tensors."""
        last = None

        @staticmethod
        def forward(ctx, out, labels, set_mask=None):
            r = _loss_call(_lib.Side(out.device), out.detach(), labels.detach(), None if set_mask is None else set_mask.detach(), True)
            ctx.save_for_backward(r["grad"])
            HeatmapMSE.last = {k: r[k] for k in ("acc", "preds", "gt", "dists")}
            return r["loss"][0].to(torch.float32)

        @staticmethod
        def backward(ctx, grad_output):
            (grad,) = ctx.saved_tensors
            return grad * grad_output.to(grad.dtype), None, None

    return HeatmapMSE


def __getattr__(name):     # HeatmapMSE is built on first use, so importing this module does not import torch
    if name == "HeatmapMSE":
        cls = _heatmap_mse_class()
        globals()["HeatmapMSE"] = cls
        return cls
    raise AttributeError(name)


# ------------------------------------------------------------------------------------------------ draws and windows
def draw_augmentation(rng, B, train=True, rotate=40, scale_factor=(0.2, 0.3)):
    """The reference's per-sample draws (pose.py:21-24, 36, 129-138) for ``B`` samples from ``rng``
    (``numpy.random.default_rng(seed)``): a dict of ``gains`` [B, 3] float32 ``U(0.7, 1.3)``, ``scale_rate`` [B] float64
    ``U(*scale_factor)``, ``flip`` [B] uint8 (probability 0.5) and ``angle`` [B] float64
    ``clip(N(0, 1) * rotate, -2 rotate, 2 rotate)``, zeroed with probability 0.6.  With ``train=False`` ``gains`` is
    None and nothing is flipped or rotated; ``scale_rate`` is still drawn, as the reference draws it.  The
    distributions are the reference's; the numbers are this generator's, not Python's ``random`` stream."""
    B = int(B)
    scale_rate = rng.uniform(float(scale_factor[0]), float(scale_factor[1]), B)
    if not train:
        return {"gains": None, "scale_rate": scale_rate, "flip": np.zeros(B, np.uint8), "angle": np.zeros(B, np.float64)}
    gains = rng.uniform(0.7, 1.3, (B, 3)).astype(np.float32)
    flip = (rng.uniform(0.0, 1.0, B) < 0.5).astype(np.uint8)
    angle = np.clip(rng.standard_normal(B) * float(rotate), -2.0 * rotate, 2.0 * rotate)
    angle[rng.uniform(0.0, 1.0, B) < 0.6] = 0.0
    return {"gains": gains, "scale_rate": scale_rate, "flip": flip, "angle": np.ascontiguousarray(angle, np.float64)}


def joint_count(parts, ul, br):
    """The reference's ``jointNum`` [B] int32: the parts with ``x > 0`` that lie strictly inside their window."""
    p = np.asarray(parts, dtype=np.float64)
    ul = np.asarray(ul, dtype=np.float32).reshape(-1, 1, 2).astype(np.float64)
    br = np.asarray(br, dtype=np.float32).reshape(-1, 1, 2).astype(np.float64)
    inside = (p[..., 0] > 0) & (p[..., 0] > ul[..., 0]) & (p[..., 1] > ul[..., 1]) & (p[..., 0] < br[..., 0]) & (p[..., 1] < br[..., 1])
    return inside.sum(axis=1).astype(np.int32)


DPG_NORMALS = ((-0.0142, 0.1158), (0.0043, 0.068), (0.0154, 0.1337), (-0.0013, 0.0711))     # pose.py:61-67


def dpg_draws(rng, B):
    """Every draw the ``opt.addDPG`` branch can ask for, for ``B`` samples: ``patch_scale`` [B], ``patch_pos`` [B, 2]
    (all ``U(0, 1)``), ``normal`` [B, 4] (xmin, ymin, xmax, ymax jitters, ``N(mu, sigma)`` of DPG_NORMALS) and
    ``switch`` [B] ``U(0, 1)``.  All are drawn whether a sample uses them or not."""
    return {"patch_scale": rng.uniform(0.0, 1.0, B), "patch_pos": rng.uniform(0.0, 1.0, (B, 2)),
            "normal": np.stack([rng.normal(mu, sd, B) for mu, sd in DPG_NORMALS], axis=1), "switch": rng.uniform(0.0, 1.0, B)}


def dpg_windows(rng, ul, br, parts, image_size, train=True, draws=None, bndbox=None):
    """The ``opt.addDPG`` branch of generateSampleBox on the windows of kpd_windows: the ``PatchScale > 0.85`` patch or
    the four normal jitters with their clamps (pose.py:44-72), then, for a training sample with ``jointNum > 13``, the
    halvings of pose.py:83-105 -- all in the reference's float32.  ``bndbox`` [B, 4] are the boxes kpd_windows widened:
    the reference scales its patch and its jitters by the height and width of the truncated box, not of the window
    (without ``bndbox`` the window's own are used).  ``draws`` (dpg_draws' dict, default: drawn from ``rng``) lets a
    caller hand in recorded draws.  ``(ul [B, 2], br [B, 2], joint_num [B])``: ``joint_num`` is counted between the two
    steps, as the reference counts it (and uses it to blank a sample afterwards)."""
    f = np.float32
    ul = np.array(ul, dtype=np.float32).reshape(-1, 2)
    br = np.array(br, dtype=np.float32).reshape(-1, 2)
    B = len(ul)
    d = dpg_draws(rng, B) if draws is None else draws
    imght, imgwidth = int(image_size[0]), int(image_size[1])
    if bndbox is None:
        hts, widths = br[:, 1] - ul[:, 1], br[:, 0] - ul[:, 0]
    else:
        box = np.trunc(np.asarray(bndbox, dtype=np.float64).reshape(-1, 4)).astype(np.float32)
        hts, widths = box[:, 3] - box[:, 1], box[:, 2] - box[:, 0]
    for b in range(B):
        ht, width = hts[b], widths[b]
        ps = float(d["patch_scale"][b])
        if ps > 0.85:
            ratio = ht / width
            if width < ht:
                pw = f(ps) * width
                ph = pw * ratio
            else:
                ph = f(ps) * ht
                pw = ph / ratio
            xmin = ul[b, 0] + f(d["patch_pos"][b, 0]) * (width - pw)
            ymin = ul[b, 1] + f(d["patch_pos"][b, 1]) * (ht - ph)
            xmax = (xmin + pw) + f(1)
            ymax = (ymin + ph) + f(1)
        else:
            n = d["normal"][b]
            xmin = max(f(1), min(ul[b, 0] + f(n[0]) * width, f(imgwidth - 3)))
            ymin = max(f(1), min(ul[b, 1] + f(n[1]) * ht, f(imght - 3)))
            xmax = min(max(xmin + f(2), br[b, 0] + f(n[2]) * width), f(imgwidth - 3))
            ymax = min(max(ymin + f(2), br[b, 1] + f(n[3]) * ht), f(imght - 3))
        ul[b] = (xmin, ymin)
        br[b] = (xmax, ymax)
    jn = joint_count(parts, ul, br)
    two = f(2)
    for b in range(B):
        if not (train and jn[b] > 13):
            continue
        sw = float(d["switch"][b])
        mx, my = (ul[b, 0] + br[b, 0]) / two, (ul[b, 1] + br[b, 1]) / two
        if sw > 0.96:
            br[b] = (mx, my)
        elif sw > 0.92:
            ul[b, 0], br[b, 1] = mx, my
        elif sw > 0.88:
            ul[b, 1], br[b, 0] = my, mx
        elif sw > 0.84:
            ul[b] = (mx, my)
        elif sw > 0.80:
            br[b, 0] = mx
        elif sw > 0.76:
            ul[b, 0] = mx
        elif sw > 0.72:
            br[b, 1] = my
        elif sw > 0.68:
            ul[b, 1] = my
    return ul, br, jn


def save_npz(path, arrays):
    """``np.savez_compressed``'s format with every member stamped 1980-01-01 and the names sorted, so the bytes depend
    on the arrays alone."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


# ------------------------------------------------------------------------------------------------ loader
class KPDSampleLoader:
    """Iterate ``(inps [b, 3, inpH, inpW], labels [b, Kp, resH, resW], setMask)`` over the annotations of
    ``annot_npz`` (annotate.write_annotations' ``annot_train.npz`` / ``annot_eval.npz``: ``bndbox`` [N, 1, 4],
    ``imgname`` [N, L], ``part`` [N, Kp, 2]) with the frames under ``img_folder``, ``batch`` samples at a time (the last
    batch may be smaller).  The frames are decoded ahead by FrameLoader (BGR, reversed to RGB here); per batch the chain
    is kpd_windows (-> dpg_windows) -> kpd_targets -> kpd_inputs -> augment_maps on inputs and labels.  ``train``
    shuffles the annotations with ``seed`` and draws the augmentation; the evaluation mode takes them in order and draws
    only ``scale_rate``.  With a ``device`` the three results are tensors on it, else numpy arrays from the host twins;
    the same seed gives the same bits either way.  ``last`` holds the draws and windows of the batch just yielded."""

    def __init__(self, annot_npz, img_folder, batch, train=True, seed=0, add_dpg=False, device=None, in_res=(320, 256),
                 out_res=(80, 64), sigma=1, rotate=40, scale_factor=(0.2, 0.3), flip_pairs=(), threads=8, depth=16):
        a = np.load(annot_npz)
        self.bndbox = np.asarray(a["bndbox"], dtype=np.float64).reshape(-1, 4)
        self.part = np.asarray(a["part"], dtype=np.float64)
        self.names = ["".join(chr(int(c)) for c in row).strip("\x00 ") for row in np.asarray(a["imgname"])]
        if not (len(self.bndbox) == len(self.part) == len(self.names)) or self.part.ndim != 3:
            raise ValueError("%s: bndbox, imgname and part disagree" % annot_npz)
        self.img_folder, self.batch, self.train, self.seed = img_folder, int(batch), bool(train), int(seed)
        if self.batch < 1:
            raise ValueError("batch must be positive")
        self.add_dpg, self.device = bool(add_dpg), device
        self.in_res, self.out_res, self.sigma = tuple(in_res), tuple(out_res), sigma
        self.rotate, self.scale_factor, self.flip_pairs = rotate, tuple(scale_factor), tuple(flip_pairs)
        self.threads, self.depth = threads, max(int(depth), 2)
        self.epoch = 0
        self.last = None

    def __len__(self):
        return (len(self.names) + self.batch - 1) // self.batch

    def _batch(self, rng, ids, frames):
        H, W = frames.shape[1:3]
        B = len(ids)
        draws = draw_augmentation(rng, B, self.train, self.rotate, self.scale_factor)
        parts = np.ascontiguousarray(self.part[ids])
        ul, br = kpd_windows(self.bndbox[ids], draws["scale_rate"], (H, W))
        if self.add_dpg:
            dd = dpg_draws(rng, B)
            ul, br, jn = dpg_windows(rng, ul, br, parts, (H, W), self.train, dd, self.bndbox[ids])
            draws.update(dpg=dd)
        else:
            jn = joint_count(parts, ul, br)
        dev = self.device
        labels, _, mask = kpd_targets(parts, ul, br, self.in_res, self.out_res, self.sigma, want_mask=True, device=dev,
                                      as_tensor=dev is not None)
        inps = kpd_inputs(frames, np.arange(B, dtype=np.int32), ul, br, draws["gains"], jn == 0, self.in_res, dev)
        if self.train:
            inps = augment_maps(inps, draws["flip"], draws["angle"], (), dev)
            labels = augment_maps(labels, draws["flip"], draws["angle"], self.flip_pairs, dev)
        self.last = dict(draws, ids=np.asarray(ids), ul=ul, br=br, joint_num=jn)
        return inps, labels, mask

    def __iter__(self):
        from .frame_loader import FrameLoader
        N = len(self.names)
        rng = np.random.default_rng([self.seed, self.epoch])
        self.epoch += 1
        order = rng.permutation(N) if self.train else np.arange(N)
        if N == 0:
            return
        loader = FrameLoader([os.path.join(self.img_folder, self.names[i]) for i in order], threads=self.threads,
                             depth=self.depth, pinned=False)
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
