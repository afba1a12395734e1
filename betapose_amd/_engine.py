"""What ``Darknet`` and ``FastPoseHIP`` share: the Python side of an engine handle of libbetapose_hip.so (``bp_yolo_*`` /
``bp_kpd_*``, include/betapose_hip.h).  A subclass names the prefix of its C entry points in ``_C`` and creates the
handle in ``_ensure``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


class _Engine:
    _C = ""            # bp_yolo / bp_kpd
    _h = None

    def _fn(self, name: str):
        return getattr(_lib.lib(), "%s_%s" % (self._C, name))

    def _call(self, name: str, *args):
        _lib.check(self._fn(name)(self._h, *args))

    def _destroy(self):
        if self._h is not None:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    @property
    def handle(self):
        self._ensure()
        return self._h

    def cuda(self, device=None):
        if device is not None:
            self._device = int(device) if not hasattr(device, "index") else device.index
        self._ensure()
        return self

    def eval(self):
        self.training = False
        return self

    def _on_device(self, x):
        """The half of ``_prep`` behind the shape check: batch bound, then f32, contiguous, on the engine's device."""
        import torch
        if x.shape[0] > self.max_batch:
            raise ValueError("batch %d > max_batch %d" % (x.shape[0], self.max_batch))
        return x.to(device="cuda:%d" % self._device, dtype=torch.float32).contiguous()

    # ---- inspection hooks (tests)
    def taps(self):
        self._ensure()
        out = []
        name = C.create_string_buffer(64)
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        for i in range(self._fn("tap_count")(self._h)):
            self._call("tap_info", i, name, 64, C.byref(c), C.byref(h), C.byref(w))
            out.append((name.value.decode(), c.value, h.value, w.value))
        return out

    def tap(self, i: int, batch: int = 1):
        import torch
        name, c, h, w = self.taps()[i]
        t = torch.empty((batch, c, h, w), device="cuda:%d" % self._device, dtype=torch.float32)
        self._call("tap_copy", i, batch, t.data_ptr(), _lib.current_stream())
        return t

    def set_policy(self, sk_target_blocks: int = 512, sk_min_chunks: int = 4, sk_max_splits: int = 8,
                   force_tile: int = -1):
        self._ensure()
        self._call("set_policy", sk_target_blocks, sk_min_chunks, sk_max_splits, force_tile)

    def set_precision(self, precision: str = "bf16x3"):
        """'f32' (fp32 MFMA), 'bf16x3' (fp32-accurate: exact 3-way bf16 operand split on the bf16 MFMA) or 'f16'
        (fp16 operands, fp32 accumulate: carries fp16 rounding); 'f16r' = 'f16' with fp16 skip connections (residuals read from the fp16
        operand planes, fp32 copies of tensors that only convolutions and residual adds read are dropped)."""
        self._ensure()
        self._call("set_precision", {"f32": 0, "f16": 1, "bf16x3": 2, "f16r": 3}[precision])
        self._precision = precision
        return self

    def clone(self):
        """Second engine over the same device filters (own activations): one per concurrent stream."""
        import copy
        self._ensure()
        h = C.c_void_p()
        self._call("clone", C.byref(h))   # first: a failed clone must not leave a copy owning self._h
        other = copy.copy(self)
        other._h = h
        return other

    def profile(self, batch: int = 1, iters: int = 10):
        """Eager pass with hipEvent pairs per op -> (ms[n_ops], info[n_ops,4] = is_conv, tile, vec, splits)."""
        self._ensure()
        fn = self._fn("profile")
        n = fn(self._h, batch, iters, None, None, 0, _lib.current_stream())
        ms = (C.c_float * n)()
        info = (C.c_int * (4 * n))()
        rc = fn(self._h, batch, iters, ms, info, n, _lib.current_stream())
        if rc < 0:
            _lib.check(rc)
        return np.array(ms, dtype=np.float64), np.array(info, dtype=np.int64).reshape(n, 4)

    def set_prefetch(self, on: bool = True):
        """Lone-frame latency mode (include/betapose_hip.h bp_*_set_prefetch): split-K hand-off inside one XCD's L2 +
        prefetch of the next layer's filters.  Bit-identical results; pays with one frame at a time, costs with several in flight."""
        self._ensure()
        self._call("set_prefetch", int(bool(on)))
        self._latency_mode = bool(on)

    def set_fusion(self, on: bool = True):
        """Conv -> conv fusion of whole residual / bottleneck blocks (include/betapose_hip.h bp_*_set_fusion; default on)."""
        self._ensure()
        self._call("set_fusion", int(bool(on)))

    def fused_launches(self, batch: int = 1) -> int:
        self._ensure()
        n = C.c_int(0)
        self._call("fused_launches", int(batch), C.byref(n))
        return int(n.value)

    def xcd_errors(self) -> int:
        """Non-zero when a launch of the latency mode found a K slice on the wrong XCD since the last call (include/betapose_hip.h
        bp_*_xcd_errors): its tile was not stored, the frame must be run again with the mode off.  Waits for the current stream."""
        if not getattr(self, "_latency_mode", False) or self._h is None:
            return 0
        n = C.c_int(0)
        self._call("xcd_errors", C.byref(n), _lib.current_stream())
        return int(n.value)

    def set_stamps(self, buf=None, slots: int = 0):
        """In-situ conv timing (include/betapose_hip.h bp_*_set_stamps): ``buf`` a cuda int64 tensor of
        n_convs * slots * 8 elements, or None to switch it off."""
        self._ensure()
        self._call("set_stamps", buf.data_ptr() if buf is not None else None, int(slots))

    def op_names(self):
        """[(layer name, is_convolution)] in op order."""
        self._ensure()
        n = self._fn("op_stats")(self._h, None, None, 0)
        name = C.create_string_buffer(96)
        out = []
        for i in range(n):
            is_conv = self._fn("op_name")(self._h, i, name, 96)
            out.append((name.value.decode(), bool(is_conv == 1)))
        return out

    def op_stats(self):
        self._ensure()
        n = self._fn("op_stats")(self._h, None, None, 0)
        f = (C.c_double * n)()
        b = (C.c_double * n)()
        self._fn("op_stats")(self._h, f, b, n)
        return np.array(f), np.array(b)
