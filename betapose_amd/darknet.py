"""``Darknet`` -- the detector, same call surface as the reference's
``yolo/darknet.py:Darknet`` (3_6Dpose_estimator/yolo/darknet.py:209-432) so that
``DetectionLoader`` (dataloader.py:285-301) runs with only its import changed:

    det_model = Darknet("yolo/cfg/yolov3-single.cfg", reso=416)
    det_model.load_weights("models/yolo/01.weights")
    det_model.net_info['height'] = 416
    det_model.cuda(); det_model.eval()
    prediction = det_model(img)            # f32[B,3,R,R] -> f32[B, sum 3g^2, 5+C]

All arithmetic runs in libbetapose_hip.so (hand-written HIP for gfx950); this class
only parses the cfg, reads the ``.weights`` file and moves pointers.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _lib
from ._engine import _Engine
from .cfg import parse_cfg, parse_cfg_text, yolov3_single_cfg_text
from .weights import darknet_stream_size, read_darknet_weights


def _cfg_text(blocks) -> str:
    out = []
    for b in blocks:
        out.append("[%s]" % b["type"])
        for k, v in b.items():
            if k != "type":
                out.append("%s=%s" % (k, v))
        out.append("")
    return "\n".join(out)


def check_class_ids(class_ids, n_classes: int, num_classes: int = 80):
    """The class list of one shared detector pass (``forward_select_classes``, ``ScenePipeline``): 1 to
    ``_lib.MAX_SCENE_CLASSES`` distinct ids, each below the class count the select compares over,
    ``min(num_classes, n_classes)`` (``n_classes``: the cfg's).  Returns the ids as a list of ints; raises ``ValueError``
    otherwise -- the library refuses the same lists (csrc/yolo_tail.hip make_class_list)."""
    ids = [int(c) for c in class_ids]
    if not 1 <= len(ids) <= _lib.MAX_SCENE_CLASSES:
        raise ValueError("class list: %d class ids, one detector pass selects for 1 to %d" % (len(ids), _lib.MAX_SCENE_CLASSES))
    if len(set(ids)) != len(ids):
        raise ValueError("class list: duplicate class ids in %s" % ids)
    top = min(int(num_classes), int(n_classes))
    for c in ids:
        if not 0 <= c < top:
            raise ValueError("class list: class id %d is not below the detector's class count %d" % (c, top))
    return ids


class Darknet(_Engine):
    _C = "bp_yolo"

    def __init__(self, cfgfile: str, reso: int = 416, max_batch: int = 1, device: Optional[int] = None):
        self.blocks = parse_cfg(cfgfile)
        self.reso = int(reso)
        self.net_info = self.blocks[0]          # aliases block 0, as in the reference (darknet.py:232)
        self.max_batch = int(max_batch)
        self._device = device
        self._stream: Optional[np.ndarray] = None
        self._h = None
        self.header = None
        self.seen = 0
        self.training = False

    @property
    def n_classes(self) -> int:
        """Classes per anchor of the cfg's [yolo] layers (attrs - 5); known without an engine."""
        return int(next(b for b in self.blocks if b["type"] == "yolo")["classes"])

    # ---- nn.Module-like surface used by the reference callers
    def load_weights(self, path: str, cutoff=None):
        if cutoff is not None:
            raise NotImplementedError("cutoff is not used on the inference path")
        self.header, self.seen, flat = read_darknet_weights(path)
        self.load_stream(flat)
        return self

    def load_stream(self, flat: np.ndarray):
        need = darknet_stream_size([b for b in self.blocks if b["type"] != "net"])
        if flat.size < need:
            raise ValueError("weights stream has %d floats, cfg needs %d" % (flat.size, need))
        self._stream = np.ascontiguousarray(flat[:need], dtype=np.float32)
        self._destroy()
        return self

    def to(self, device):
        return self.cuda(device)

    def __call__(self, x, y_true=None):
        return self.forward(x)

    # ---- engine
    def _ensure(self):
        if self._h is not None:
            return
        import torch
        _lib.require_gpu()
        if self._stream is None:
            raise RuntimeError("call load_weights() before the first forward")
        if self._device is None:
            self._device = torch.cuda.current_device()
        h = C.c_void_p()
        blocks = [b for b in self.blocks if b["type"] != "net"]
        _lib.check(_lib.lib().bp_yolo_create_from_memory(
            _cfg_text(blocks).encode(), self._stream.ctypes.data, self._stream.size, self.reso, self.max_batch,
            self._device, C.byref(h)))
        self._h = h
        self.rows = _lib.lib().bp_yolo_rows(h)
        self.attrs = _lib.lib().bp_yolo_attrs(h)

    def _prep(self, x):
        self._ensure()
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != self.reso or x.shape[3] != self.reso:
            raise ValueError("expected [B,3,%d,%d], got %s" % (self.reso, self.reso, tuple(x.shape)))
        return self._on_device(x)

    def forward(self, x):
        """f32[B,3,R,R] (RGB 0..1) -> f32[B, rows, 5+C] in DetectionLayer row order."""
        import torch
        x = self._prep(x)
        pred = torch.empty((x.shape[0], self.rows, self.attrs), device=x.device, dtype=torch.float32)
        _lib.check(_lib.lib().bp_yolo_forward(self._h, x.data_ptr(), x.shape[0], pred.data_ptr(), _lib.current_stream()))
        return pred

    def forward_select(self, x, confidence: float = 0.01, num_classes: int = 80, want_pred: bool = False):
        """Fused forward + ``dynamic_write_results`` (yolo/util.py:104-223, NMS off):
        returns ``sel`` f32[B,8] = (idx as int bits, x1,y1,x2,y2,obj,cls_conf,cls_idx); idx=-1 -> no detection."""
        import torch
        x = self._prep(x)
        sel = torch.empty((x.shape[0], 8), device=x.device, dtype=torch.float32)
        pred = torch.empty((x.shape[0], self.rows, self.attrs), device=x.device, dtype=torch.float32) if want_pred else None
        _lib.check(_lib.lib().bp_yolo_forward_select(self._h, x.data_ptr(), x.shape[0], float(confidence), int(num_classes),
                                                     pred.data_ptr() if want_pred else None, sel.data_ptr(),
                                                     _lib.current_stream()))
        return (sel, pred) if want_pred else sel

    def forward_select_classes(self, x, class_ids, confidence: float = 0.01, num_classes: int = 80, want_pred: bool = False):
        """One pass of a multi-class detector, the best box of every class in ``class_ids`` (at most 16, distinct):
        ``write_results``' rule with the class filter generalised -- a row with objectness > confidence belongs to its
        arg-max class, per class the highest objectness wins.  Returns ``sel`` f32[B,K,8] in list order:
        ``forward_select``'s record with [6] = the class's score and [7] = the class id, idx = -1 for a class without a
        row.  ``want_pred``: also the prediction tensor (the records are then selected from it instead of decoded from
        the heads; same records)."""
        import torch
        ids = check_class_ids(class_ids, self.n_classes, num_classes)
        x = self._prep(x)
        K = len(ids)
        sel = torch.empty((x.shape[0], K, 8), device=x.device, dtype=torch.float32)
        pred = torch.empty((x.shape[0], self.rows, self.attrs), device=x.device, dtype=torch.float32) if want_pred else None
        arr = (C.c_int * K)(*ids)
        _lib.check(_lib.lib().bp_yolo_forward_select_classes(self._h, x.data_ptr(), x.shape[0], float(confidence), int(num_classes),
                                                             C.cast(arr, C.c_void_p), K, pred.data_ptr() if want_pred else None,
                                                             sel.data_ptr(), _lib.current_stream()))
        return (sel, pred) if want_pred else sel

    def forward_select_nms(self, x, max_candidates: int, nms_conf: float, class_id: int = 0, confidence: float = 0.01,
                           num_classes: int = 80, want_pred: bool = False):
        """Fused forward + ``write_results`` with its NMS branch live and the final arg-max removed (yolo/util.py:176-196):
        up to ``max_candidates`` (at most 8) NMS survivors of class ``class_id`` per image, by descending objectness.
        Returns ``(sel f32[B,C,8], counts int32[B])``: ``forward_select``'s record per survivor ([6] = the class's score,
        [7] = the class id), unused slots idx = -1; candidate 0 is ``forward_select``'s record.  ``want_pred``: also
        the prediction tensor (the records are then selected from it; same records)."""
        import torch
        Cn = int(max_candidates)
        if not 1 <= Cn <= _lib.MAX_CANDIDATES:
            raise ValueError("max_candidates must be 1 to %d, not %d" % (_lib.MAX_CANDIDATES, Cn))
        x = self._prep(x)
        sel = torch.empty((x.shape[0], Cn, 8), device=x.device, dtype=torch.float32)
        counts = torch.empty((x.shape[0],), device=x.device, dtype=torch.int32)
        pred = torch.empty((x.shape[0], self.rows, self.attrs), device=x.device, dtype=torch.float32) if want_pred else None
        _lib.check(_lib.lib().bp_yolo_forward_select_nms(self._h, x.data_ptr(), x.shape[0], float(confidence), int(num_classes),
                                                         int(class_id), float(nms_conf), Cn, pred.data_ptr() if want_pred else None,
                                                         sel.data_ptr(), counts.data_ptr(), _lib.current_stream()))
        return (sel, counts, pred) if want_pred else (sel, counts)


def sel_to_dets(sel) -> "object":
    """sel f32[B,8] (device or cpu) -> what ``dynamic_write_results`` returns:
    int ``0`` when no image has a detection, else f32[n,8] rows
    (batch_idx, x1,y1,x2,y2, obj, cls_conf, cls_idx)  (yolo/util.py:206-222)."""
    import torch
    s = sel.detach().cpu()
    idx = s[:, 0].contiguous().view(torch.int32)
    keep = idx >= 0
    if not bool(keep.any()):
        return 0
    rows = []
    for b in torch.nonzero(keep).flatten().tolist():
        rows.append(torch.cat((torch.tensor([float(b)]), s[b, 1:8])))
    return torch.stack(rows)
