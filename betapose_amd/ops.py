"""Stand-alone device stages of the hot path (thin ctypes wrappers, torch tensors
as device memory): fused conv (unit-test / benchmark hook), crop, Pillow-exact
bicubic resize, PnP."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib

ACT = {"linear": 0, "leaky": 1, "relu": 2}
STORE = {"nhwc": 0, "up2": 1, "pixshuf": 2, "nchw": 3}
# + 256: fp16 operands, + 512: bf16x3 (fp32-accurate) operands.  pl<BM>[x<BN>] = conv_pl.hip (operand planes + LDS-DMA);
# w<WM>x<WN> = conv_w64.hip with WM x WN waves of 64x64; kg / rd / bd: the round-2 experiments (csrc/bp_common.h ConvTile)
_F16, _B3 = 256, 512
TILE = {"auto": -1, "64x64": 0, "128x64": 1, "stem3": 20, "stem7": 28, "64x64_f16": _F16, "128x64_f16": _F16 + 1, "64x64_b3": _B3, "bd_b3": _B3 + 12,
        "bd_f16": _F16 + 12, "halo64_b3": _B3 + 21, "halo128_b3": _B3 + 22, "halo64k2_b3": _B3 + 23, "bdk2_b3": _B3 + 24}
for _n, _i in (("w1x1", 2), ("w1x2", 3), ("w2x1", 5), ("w2x2", 6), ("pl64", 13), ("pl128", 14), ("pl128x64", 15), ("pl256x128", 16), ("pl128s", 17), ("pl64k2", 18), ("pl64bd", 19), ("plh128", 25), ("s1", 26), ("p3", 27)):
    TILE[_n + "_f16"] = _F16 + _i
    TILE[_n + "_b3"] = _B3 + _i
for _n, _i in (("kg1", 7), ("kg2", 8), ("kg4", 9), ("rd4", 10), ("rd8", 11)):
    TILE[_n + "_b3"] = _B3 + _i


def conv2d_nhwc(x, weight, bias=None, stride: int = 1, pad: int = 0, act: str = "linear", store: str = "nhwc",
                res=None, res_after_act: bool = False, tile: str = "auto", splits: int = 0, iters: int = 0,
                planes: bool = False, out=None, res_scale=None, pool=False):
    """One fused convolution.  ``x``: cuda f32 [N,H,W,Cin] (NHWC); ``weight``: host
    numpy/torch [Cout,Cin,k,k]; returns the output tensor laid out per ``store`` and,
    when ``iters`` > 0, also the measured ms per launch.  ``planes``: also return the operand planes the epilogue
    emits for the next layer (int16 tensor [np, *out.shape]: np = 1 fp16 bits / 3 bf16 bits).

    ``out``: a caller-allocated output tensor (cuda f32, contiguous, the shape ``store`` gives) that the launch writes and
    the call returns, instead of a fresh one -- a caller that pre-fills it sees which elements the launch stored.

    Environment, read by the library on every call: ``BP_CONV_F16R=1`` makes an ``*_f16`` launch as the engine's ``f16r``
    plan makes it -- ``res`` is rounded to its fp16 plane and the kernel reads the skip connection from that plane
    (ConvParams::res16), and with ``planes=True`` the fp32 store is dropped (ConvParams::skip_f32): only the returned plane
    is written, the fp32 tensor keeps whatever it held (unspecified, unless the caller passed ``out``).

    ``res_scale``: cuda f32 [N, Cout], the SE gate of the skip connection -- ``res`` is multiplied by it per image and channel
    (ConvParams::res_scale; needs ``res``).  ``pool``: the launch's epilogue also writes the sums of conv + bias over every 64-row
    slab (ConvParams::pool_out) into a cuda f32 buffer [ceil(N*OH*OW / 64), Cout], returned behind the planes; ``True`` allocates
    it, a caller's tensor (contiguous f32, at least that many elements; pre-filled, it shows what the launch wrote) is used and
    returned as it is.  The library refuses the launch forms whose epilogue cannot carry the pool."""
    import torch
    _lib.require_gpu()
    w = np.ascontiguousarray(weight.detach().cpu().numpy() if hasattr(weight, "detach") else weight, dtype=np.float32)
    b = None
    if bias is not None:
        b = np.ascontiguousarray(bias.detach().cpu().numpy() if hasattr(bias, "detach") else bias, dtype=np.float32)
    N, H, W, Cin = x.shape
    Cout, _, k, _ = w.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = x.contiguous()
    if store == "nhwc":
        shape = (N, OH, OW, Cout)
    elif store == "up2":
        shape = (N, 2 * OH, 2 * OW, Cout)
    elif store == "pixshuf":
        shape = (N, 2 * OH, 2 * OW, Cout // 4)
    else:
        shape = (N, Cout, OH, OW)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    elif not (tuple(out.shape) == shape and out.dtype == torch.float32 and out.device == x.device and out.is_contiguous()):
        raise ValueError("out must be a contiguous float32 tensor of shape %s on %s" % (shape, x.device))
    ms = C.c_float(0)
    pl = None
    if planes:
        assert store != "nchw", "NCHW outputs (the heat-maps) have no operand planes"
        pl = torch.zeros((1 if TILE[tile] < _B3 else 3,) + tuple(out.shape), device=x.device, dtype=torch.int16)
    rs = None
    if res_scale is not None:
        if not (tuple(res_scale.shape) == (N, Cout) and res_scale.dtype == torch.float32 and res_scale.device == x.device):
            raise ValueError("res_scale must be a float32 tensor of shape %s on %s" % ((N, Cout), x.device))
        rs = res_scale.contiguous()
    pb = None
    if pool is not False and pool is not None:
        slabs = (N * OH * OW + 63) // 64
        if pool is True:
            pb = torch.empty((slabs, Cout), device=x.device, dtype=torch.float32)
        else:
            pb = pool
            if not (pb.dtype == torch.float32 and pb.device == x.device and pb.is_contiguous() and pb.numel() >= slabs * Cout):
                raise ValueError("pool must be a contiguous float32 tensor of at least %d elements on %s" % (slabs * Cout, x.device))
    r = res.contiguous() if res is not None else None
    _lib.check(_lib.lib().bp_conv2d_se(x.data_ptr(), N, H, W, Cin, w.ctypes.data, b.ctypes.data if b is not None else None,
                                       Cout, k, stride, pad, ACT[act], STORE[store],
                                       r.data_ptr() if r is not None else None, int(res_after_act),
                                       TILE[tile], int(splits), out.data_ptr(), pl.data_ptr() if planes else None,
                                       rs.data_ptr() if rs is not None else None, pb.data_ptr() if pb is not None else None,
                                       int(iters), C.byref(ms), _lib.current_stream()))
    ret = (out,) + ((pl,) if planes else ()) + ((pb,) if pb is not None else ()) + ((ms.value,) if iters > 0 else ())
    return ret if len(ret) > 1 else out


FC_ACT = {"linear": 0, "relu": 2, "sigmoid": 3}


def avgpool_parts(x, channels: Optional[int] = None, col0: int = 0, out=None):
    """The SE blocks' global average pool as slice sums (bp_avgpool, avgpool_partial_kernel).  ``x``: cuda f32 [N, HW, ld] (or
    [N, H, W, ld]) whose rows are contiguous; columns ``col0`` .. ``col0 + channels`` of a row are pooled (default: all, ld == C) --
    a view into a wider tensor is passed as the wide tensor plus the view's columns.  Returns (sums [N, P, C], P): the sums of P pixel
    slices of ceil(HW / P) pixels each; the mean is sums.sum(1) / HW.  ``out``: a caller's contiguous cuda f32 tensor of that shape to
    write into (pre-filled, it shows what the launch wrote)."""
    import torch
    _lib.require_gpu()
    assert x.dtype == torch.float32 and x.dim() in (3, 4)
    x = x.contiguous()
    N, ld = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * ld)
    Cc = ld - col0 if channels is None else int(channels)
    assert 0 <= col0 and Cc >= 1 and col0 + Cc <= ld
    parts = C.c_int(0)
    _lib.check(_lib.lib().bp_avgpool(None, ld, N, HW, Cc, None, C.byref(parts), _lib.current_stream()))
    if out is None:
        out = torch.empty((N, parts.value, Cc), device=x.device, dtype=torch.float32)
    elif not (tuple(out.shape) == (N, parts.value, Cc) and out.dtype == torch.float32 and out.device == x.device and out.is_contiguous()):
        raise ValueError("out must be a contiguous float32 tensor of shape %s on %s" % ((N, parts.value, Cc), x.device))
    _lib.check(_lib.lib().bp_avgpool(x.data_ptr() + 4 * col0, ld, N, HW, Cc, out.data_ptr(), C.byref(parts), _lib.current_stream()))
    return out, parts.value


def fc(x, weight, bias=None, act: str = "linear", in_scale: float = 1.0):
    """The SE blocks' fully connected layer (bp_fc, fc_kernel): act(bias + weight @ v).  ``x``: cuda f32 [N, Cin] (v = x), or
    [N, in_parts, Cin] slice sums (v = in_scale * x.sum(1)); ``weight``: host numpy/torch [Cout, Cin], Cin % 4 == 0; ``act``
    'linear' / 'relu' / 'sigmoid'.  Returns cuda f32 [N, Cout]."""
    import torch
    _lib.require_gpu()
    w = np.ascontiguousarray(weight.detach().cpu().numpy() if hasattr(weight, "detach") else weight, dtype=np.float32)
    b = None
    if bias is not None:
        b = np.ascontiguousarray(bias.detach().cpu().numpy() if hasattr(bias, "detach") else bias, dtype=np.float32)
    assert x.dtype == torch.float32 and x.dim() in (2, 3)
    x = x.contiguous()
    N, Cin = x.shape[0], x.shape[-1]
    parts = x.shape[1] if x.dim() == 3 else 1
    Cout = w.shape[0]
    assert w.shape == (Cout, Cin) and (b is None or b.shape == (Cout,))
    out = torch.empty((N, Cout), device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().bp_fc(x.data_ptr(), w.ctypes.data, b.ctypes.data if b is not None else None, N, Cin, Cout, FC_ACT[act],
                                int(parts), float(in_scale), out.data_ptr(), _lib.current_stream()))
    return out


def _aux_planes(out, planes):
    import torch
    if not planes:
        return None, 0
    npl = {"f16": 1, "b3": 3}[planes]
    return torch.zeros((npl,) + tuple(out.shape), device=out.device, dtype=torch.int16), npl


def maxpool3s2p1(x, planes: Optional[str] = None):
    """MaxPool 3x3 / stride 2 / pad 1 (bp_maxpool3s2p1): cuda f32 NHWC [N, H, W, C], C % 4 == 0 -> [N, (H-1)//2+1, (W-1)//2+1, C].
    ``planes`` 'f16' / 'b3': also return the operand planes the kernel writes for the next layer (int16 [np, *out.shape])."""
    import torch
    _lib.require_gpu()
    assert x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    N, H, W, Cc = x.shape
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), device=x.device, dtype=torch.float32)
    pl, npl = _aux_planes(out, planes)
    _lib.check(_lib.lib().bp_maxpool3s2p1(x.data_ptr(), N, H, W, Cc, out.data_ptr(), pl.data_ptr() if pl is not None else None, npl,
                                          _lib.current_stream()))
    return (out, pl) if pl is not None else out


def pixel_shuffle2(x, planes: Optional[str] = None):
    """PixelShuffle(2) (bp_pixel_shuffle2): cuda f32 NHWC [N, H, W, C], C % 4 == 0 -> [N, 2H, 2W, C/4] with torch's channel order
    (out[c, 2h+i, 2w+j] = in[4c + 2i + j, h, w]).  ``planes``: as ``maxpool3s2p1``."""
    import torch
    _lib.require_gpu()
    assert x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    N, H, W, Cc = x.shape
    out = torch.empty((N, 2 * H, 2 * W, Cc // 4), device=x.device, dtype=torch.float32)
    pl, npl = _aux_planes(out, planes)
    _lib.check(_lib.lib().bp_pixel_shuffle2(x.data_ptr(), N, H, W, Cc, out.data_ptr(), pl.data_ptr() if pl is not None else None, npl,
                                            _lib.current_stream()))
    return (out, pl) if pl is not None else out


def crop(frames_bgr_u8, sel=None, boxes=None, reso: int = 416, oh: int = 320, ow: int = 256, nchw: bool = True):
    """Device crop (dataloader.py:354-364,794-835; img.py:242-262).  ``frames``: cuda u8
    [B,H,W,3] BGR; ``sel`` [B,8] (YOLO-input-pixel boxes) or ``boxes`` [B,4] (frame pixels).
    Returns (inps [B,3,oh,ow] or [B,oh,ow,3], pts [B,8] = pt1.x,pt1.y,pt2.x,pt2.y, box x1,y1,x2,y2)."""
    import torch
    _lib.require_gpu()
    f = frames_bgr_u8.contiguous()
    B, H, W, _ = f.shape
    out = torch.empty((B, 3, oh, ow) if nchw else (B, oh, ow, 3), device=f.device, dtype=torch.float32)
    pts = torch.empty((B, 8), device=f.device, dtype=torch.float32)
    _lib.check(_lib.lib().bp_crop(f.data_ptr(), B, H, W, sel.contiguous().data_ptr() if sel is not None else None, reso,
                                  boxes.contiguous().data_ptr() if boxes is not None else None,
                                  out.data_ptr() if nchw else None, None if nchw else out.data_ptr(), pts.data_ptr(),
                                  oh, ow, _lib.current_stream()))
    return out, pts


def crop_candidates(frames_bgr_u8, candidates: int, sel=None, boxes=None, reso: int = 416, oh: int = 320, ow: int = 256,
                    nchw: bool = True):
    """``crop`` over ``candidates`` boxes per frame (bp_crop_candidates): ``frames`` cuda u8 [F,H,W,3]; ``sel`` [F*C,8] or
    ``boxes`` [F*C,4]; crop n reads frame n // C with box n.  Returns (inps [F*C,...], pts [F*C,8])."""
    import torch
    _lib.require_gpu()
    f = frames_bgr_u8.contiguous()
    F, H, W, _ = f.shape
    Cn = int(candidates)
    B = F * Cn
    src = sel if sel is not None else boxes
    src = src.contiguous().reshape(B, -1)
    assert src.shape[1] == (8 if sel is not None else 4)
    out = torch.empty((B, 3, oh, ow) if nchw else (B, oh, ow, 3), device=f.device, dtype=torch.float32)
    pts = torch.empty((B, 8), device=f.device, dtype=torch.float32)
    _lib.check(_lib.lib().bp_crop_candidates(f.data_ptr(), F, Cn, H, W, src.data_ptr() if sel is not None else None, reso,
                                             src.data_ptr() if sel is None else None,
                                             out.data_ptr() if nchw else None, None if nchw else out.data_ptr(), pts.data_ptr(),
                                             oh, ow, _lib.current_stream()))
    return out, pts


def select(pred, confidence: float = 0.01, num_classes: int = 80):
    """The plain select on an existing prediction tensor (bp_yolo_select): cuda f32 [B,rows,attrs] -> sel f32 [B,8], per
    image the arg-max objectness row above ``confidence`` whose arg-max class is 0."""
    import torch
    _lib.require_gpu()
    p = pred.contiguous()
    assert p.dtype == torch.float32 and p.dim() == 3
    B, rows, attrs = p.shape
    sel = torch.empty((B, 8), device=p.device, dtype=torch.float32)
    _lib.check(_lib.lib().bp_yolo_select(p.data_ptr(), B, rows, attrs, float(confidence), int(num_classes), sel.data_ptr(),
                                         _lib.current_stream()))
    return sel


def select_nms(pred, max_candidates: int, nms_conf: float, class_id: int = 0, confidence: float = 0.01, num_classes: int = 80):
    """Select with box NMS on an existing prediction tensor (bp_yolo_select_nms): cuda f32 [B,rows,attrs] ->
    (sel f32 [B,C,8], counts int32 [B]); see ``Darknet.forward_select_nms``."""
    import torch
    _lib.require_gpu()
    p = pred.contiguous()
    assert p.dtype == torch.float32 and p.dim() == 3
    B, rows, attrs = p.shape
    Cn = int(max_candidates)
    sel = torch.empty((B, Cn, 8), device=p.device, dtype=torch.float32)
    counts = torch.empty((B,), device=p.device, dtype=torch.int32)
    _lib.check(_lib.lib().bp_yolo_select_nms(p.data_ptr(), B, rows, attrs, float(confidence), int(num_classes), int(class_id),
                                             float(nms_conf), Cn, sel.data_ptr(), counts.data_ptr(), _lib.current_stream()))
    return sel, counts


def pose_from_candidate_records(records, counts, kp3d, K, left_number: int = 50):
    """The candidate pose tail on records made any way (bp_pose_from_candidate_records): cuda f32 [F,C,316] and int32 [F]
    -> (poses f64 [F,166], merged f32 [F,C,152], info int32 [F,4]); layouts: include/betapose_hip.h."""
    import torch
    _lib.require_gpu()
    rec = records.contiguous()
    assert rec.dtype == torch.float32 and rec.dim() == 3 and rec.shape[2] == _lib.RESULT_FLOATS
    F, Cn = rec.shape[0], rec.shape[1]
    cnt = counts.to(device=rec.device, dtype=torch.int32).contiguous()
    assert cnt.shape == (F,)
    k3 = torch.as_tensor(np.asarray(kp3d, dtype=np.float64).reshape(-1, 3), device=rec.device).contiguous()
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    poses = torch.empty((F, _lib.POSE_DOUBLES), dtype=torch.float64, device=rec.device)
    merged = torch.zeros((F, Cn, _lib.MERGED_FLOATS), dtype=torch.float32, device=rec.device)
    info = torch.zeros((F, 4), dtype=torch.int32, device=rec.device)
    _lib.check(_lib.lib().bp_pose_from_candidate_records(rec.data_ptr(), cnt.data_ptr(), F, Cn, k3.data_ptr(), k3.shape[0],
                                                         Kc.ctypes.data, int(left_number), poses.data_ptr(), merged.data_ptr(),
                                                         info.data_ptr(), _lib.current_stream()))
    return poses, merged, info


def pose_instances(merged, info, poses, kp3d, K, left_number: int = 50):
    """A pose for every merged candidate (bp_pose_instances_from_merged) on ``pose_from_candidate_records``' outputs: cuda
    merged f32 [F,C,152], info int32 [F,4], poses f64 [F,166] -> f64 [F,C,166]: row 0 is the frame's pose row, row
    0 < j < m the pruned PnP of merged pose j, every other row status 1; layouts: include/betapose_hip.h."""
    import torch
    _lib.require_gpu()
    mg = merged.contiguous()
    assert mg.dtype == torch.float32 and mg.dim() == 3 and mg.shape[2] == _lib.MERGED_FLOATS
    F, Cn = mg.shape[0], mg.shape[1]
    inf = info.to(device=mg.device, dtype=torch.int32).contiguous()
    ps = poses.to(device=mg.device, dtype=torch.float64).contiguous()
    assert inf.shape == (F, 4) and ps.shape == (F, _lib.POSE_DOUBLES)
    k3 = torch.as_tensor(np.asarray(kp3d, dtype=np.float64).reshape(-1, 3), device=mg.device).contiguous()
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    inst = torch.empty((F, Cn, _lib.POSE_DOUBLES), dtype=torch.float64, device=mg.device)
    _lib.check(_lib.lib().bp_pose_instances_from_merged(mg.data_ptr(), inf.data_ptr(), ps.data_ptr(), F, Cn, k3.data_ptr(),
                                                        k3.shape[0], Kc.ctypes.data, int(left_number), inst.data_ptr(),
                                                        _lib.current_stream()))
    return inst


def resize_bicubic(frames_u8, oh: int = 416, ow: int = 416, swap_rb: bool = True, want: str = "f32"):
    """Pillow-exact antialiased bicubic (dataloader.py:94-99).  ``frames``: cuda u8 [B,H,W,3].
    ``want`` 'u8' -> u8 [B,oh,ow,3]; 'f32' -> f32 NHWC /255."""
    import torch
    _lib.require_gpu()
    f = frames_u8.contiguous()
    B, H, W, _ = f.shape
    if want == "u8":
        out = torch.empty((B, oh, ow, 3), device=f.device, dtype=torch.uint8)
        _lib.check(_lib.lib().bp_resize_bicubic(f.data_ptr(), B, H, W, oh, ow, int(swap_rb), out.data_ptr(), None,
                                                _lib.current_stream()))
    else:
        out = torch.empty((B, oh, ow, 3), device=f.device, dtype=torch.float32)
        _lib.check(_lib.lib().bp_resize_bicubic(f.data_ptr(), B, H, W, oh, ow, int(swap_rb), None, out.data_ptr(),
                                                _lib.current_stream()))
    return out


def solve_pnp(points_3d, points_2d, K, method: str = "iterative"):
    """utils/utils.py:17-41 ``pnp``: returns (R [3,3], t [3,1]) f64.  Host-only (no GPU needed).
    ``method``: 'iterative' = the restatement of cv2.solvePnP's SOLVEPNP_ITERATIVE (what the reference calls);
    'refined' = conditioned DLT + converged minimiser (opt-in, csrc/host_post.cpp)."""
    p3 = np.ascontiguousarray(points_3d, dtype=np.float64)
    p2 = np.ascontiguousarray(np.asarray(points_2d)[:, :2], dtype=np.float64)
    assert p3.shape[0] == p2.shape[0], "points 3D and points 2D must have same number of vertices"
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    R = np.empty((3, 3), np.float64)
    t = np.empty(3, np.float64)
    fn = {"iterative": _lib.lib().bp_solve_pnp, "refined": _lib.lib().bp_solve_pnp_refined}[method]
    _lib.check(fn(p3.ctypes.data, p2.ctypes.data, p3.shape[0], Kc.ctypes.data, R.ctypes.data, t.ctypes.data))
    return R, t.reshape(3, 1)


def solve_pnp_status(points_3d, points_2d, K):
    """``solve_pnp`` with a failure reported instead of raised (bp_solve_pnp_status): returns (R, t, status); status 0 =
    solved, else the solver's code (-1 too few points, -2 degenerate) and R, t are empty lists."""
    p3 = np.ascontiguousarray(points_3d, dtype=np.float64)
    p2 = np.ascontiguousarray(np.asarray(points_2d)[:, :2], dtype=np.float64)
    assert p3.shape[0] == p2.shape[0], "points 3D and points 2D must have same number of vertices"
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    R = np.empty((3, 3), np.float64)
    t = np.empty(3, np.float64)
    st = C.c_int(0)
    _lib.check(_lib.lib().bp_solve_pnp_status(p3.ctypes.data, p2.ctypes.data, p3.shape[0], Kc.ctypes.data, R.ctypes.data,
                                              t.ctypes.data, C.addressof(st)))
    if st.value != 0:
        return [], [], int(st.value)
    return R, t.reshape(3, 1), 0


def solve_pnp_batch(points_3d, points_2d, K):
    """``solve_pnp`` over P independent problems in one device launch (bp_solve_pnp_batch, one wave per problem).
    ``points_3d``: [n,3] shared by every problem or [P,n,3]; ``points_2d``: [P,n,2]; numpy or torch, n <= 64.  Returns
    (R [P,3,3], t [P,3,1], status [P] int32) as cuda torch tensors: status 0 = solved, -1 too few points, -2 degenerate
    (R, t NaN there), the codes of the host solver."""
    import torch
    _lib.require_gpu()
    p2 = torch.as_tensor(points_2d, dtype=torch.float64).cuda().contiguous()
    assert p2.dim() == 3 and p2.shape[2] >= 2, "points_2d must be [P, n, 2]"
    p2 = p2[:, :, :2].contiguous()
    P, n = p2.shape[0], p2.shape[1]
    p3 = torch.as_tensor(points_3d, dtype=torch.float64).to(p2.device).contiguous()
    shared = p3.dim() == 2
    assert p3.shape[-2:] == (n, 3) and (shared or p3.shape[0] == P), "points 3D and points 2D must have same number of vertices"
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    Rt = torch.empty((P, 3, 4), dtype=torch.float64, device=p2.device)
    st = torch.empty(P, dtype=torch.int32, device=p2.device)
    _lib.check(_lib.lib().bp_solve_pnp_batch(p3.data_ptr(), int(shared), p2.data_ptr(), n, P, Kc.ctypes.data,
                                             Rt.data_ptr(), st.data_ptr(), _lib.current_stream()))
    return Rt[:, :, :3].contiguous(), Rt[:, :, 3:].contiguous(), st


def pose_from_records(records, kp3d, K, left_number: int = 50):
    """The device pose tail on records made any way (bp_pose_from_records): cuda f32 [B,316] -> cuda f64 [B,166]."""
    import torch
    _lib.require_gpu()
    rec = records.contiguous()
    assert rec.dtype == torch.float32 and rec.dim() == 2 and rec.shape[1] == _lib.RESULT_FLOATS
    k3 = torch.as_tensor(np.asarray(kp3d, dtype=np.float64).reshape(-1, 3), device=rec.device).contiguous()
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    out = torch.empty((rec.shape[0], _lib.POSE_DOUBLES), dtype=torch.float64, device=rec.device)
    _lib.check(_lib.lib().bp_pose_from_records(rec.data_ptr(), rec.shape[0], k3.data_ptr(), k3.shape[0], Kc.ctypes.data,
                                               int(left_number), out.data_ptr(), _lib.current_stream()))
    return out


def solve_pnp_ransac(points_3d, points_2d, K, reprojection_error: float = 12.0, iterations: int = 100,
                     confidence: float = 0.99):
    """The variant utils/utils.py:32-36 keeps commented out (cv2.solvePnPRansac, reprojectionError=12.0): returns
    (R [3,3], t [3,1], inlier mask [n] bool).  Host-only."""
    p3 = np.ascontiguousarray(points_3d, dtype=np.float64)
    p2 = np.ascontiguousarray(np.asarray(points_2d)[:, :2], dtype=np.float64)
    assert p3.shape[0] == p2.shape[0], "points 3D and points 2D must have same number of vertices"
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    R = np.empty((3, 3), np.float64)
    t = np.empty(3, np.float64)
    inl = np.zeros(p3.shape[0], np.uint8)
    _lib.check(_lib.lib().bp_solve_pnp_ransac(p3.ctypes.data, p2.ctypes.data, p3.shape[0], Kc.ctypes.data,
                                              float(reprojection_error), int(iterations), float(confidence),
                                              R.ctypes.data, t.ctypes.data, inl.ctypes.data))
    return R, t.reshape(3, 1), inl.astype(bool)


def pnp_ransac_samples(n: int, max_trials: int = 100):
    """The draws of ``solve_pnp_ransac``'s sampler (bp_pnp_ransac_samples): int32 [max_trials, 6], six distinct indices
    below ``n`` per trial.  They depend on (n, max_trials) alone; host and device solver read this one table."""
    idx = np.empty((int(max_trials), 6), np.int32)
    _lib.check(_lib.lib().bp_pnp_ransac_samples(int(n), int(max_trials), idx.ctypes.data))
    return idx


def pnp_ransac_trials_needed(n: int, confidence: float = 0.99):
    """The early stop of ``solve_pnp_ransac`` as a table (bp_pnp_ransac_trials_needed): int32 [n + 1], the trial limit
    after a hypothesis with ``cnt`` inliers (INT_MAX: none)."""
    need = np.empty(int(n) + 1, np.int32)
    _lib.check(_lib.lib().bp_pnp_ransac_trials_needed(int(n), float(confidence), need.ctypes.data))
    return need


def solve_pnp_ransac_batch(points_3d, points_2d, K, reprojection_error: float = 12.0, iterations: int = 100,
                           confidence: float = 0.99, workspace=None):
    """``solve_pnp_ransac`` over P independent problems on the device (bp_solve_pnp_ransac_batch): every hypothesis of
    every problem is one wave, then one wave per problem replays the host's trial loop and refits on the inliers -- the
    result is the host loop's.  Arguments as ``solve_pnp_batch``.  Returns (Rt [P,3,4] f64, status [P] int32, inliers
    [P,n] bool) as cuda tensors: status 0 solved, -1 fewer than six points, -2 no six-point consensus or a degenerate
    refit (Rt NaN there).  ``workspace``: a cuda uint8 tensor to reuse between calls (default: allocated here)."""
    import torch
    _lib.require_gpu()
    p2 = torch.as_tensor(points_2d, dtype=torch.float64).cuda().contiguous()
    assert p2.dim() == 3 and p2.shape[2] >= 2, "points_2d must be [P, n, 2]"
    p2 = p2[:, :, :2].contiguous()
    P, n = p2.shape[0], p2.shape[1]
    p3 = torch.as_tensor(points_3d, dtype=torch.float64).to(p2.device).contiguous()
    shared = p3.dim() == 2
    assert p3.shape[-2:] == (n, 3) and (shared or p3.shape[0] == P), "points 3D and points 2D must have same number of vertices"
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    Rt = torch.empty((P, 3, 4), dtype=torch.float64, device=p2.device)
    st = torch.empty(P, dtype=torch.int32, device=p2.device)
    inl = torch.empty((P, n), dtype=torch.uint8, device=p2.device)
    if workspace is None:
        nbytes = int(_lib.lib().bp_pnp_ransac_workspace_bytes(P, max(int(iterations), 1)))
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=p2.device)
    _lib.check(_lib.lib().bp_solve_pnp_ransac_batch(p3.data_ptr(), int(shared), p2.data_ptr(), n, P, Kc.ctypes.data,
                                                    float(reprojection_error), int(iterations), float(confidence),
                                                    Rt.data_ptr(), st.data_ptr(), inl.data_ptr(), workspace.data_ptr(),
                                                    workspace.numel(), _lib.current_stream()))
    return Rt, st, inl.bool()


def pose_from_records_ransac(records, kp3d, K, left_number: int = 50, reprojection_error: float = 12.0,
                             iterations: int = 100, confidence: float = 0.99):
    """``pose_from_records`` with the RANSAC solver (bp_pose_from_records_ransac): slot 15 of a row is the inlier set."""
    import torch
    _lib.require_gpu()
    rec = records.contiguous()
    assert rec.dtype == torch.float32 and rec.dim() == 2 and rec.shape[1] == _lib.RESULT_FLOATS
    k3 = torch.as_tensor(np.asarray(kp3d, dtype=np.float64).reshape(-1, 3), device=rec.device).contiguous()
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    out = torch.empty((rec.shape[0], _lib.POSE_DOUBLES), dtype=torch.float64, device=rec.device)
    nbytes = int(_lib.lib().bp_pose_ransac_workspace_bytes(rec.shape[0], max(int(iterations), 1)))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=rec.device)
    _lib.check(_lib.lib().bp_pose_from_records_ransac(rec.data_ptr(), rec.shape[0], k3.data_ptr(), k3.shape[0], Kc.ctypes.data,
                                                      int(left_number), float(reprojection_error), int(iterations),
                                                      float(confidence), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      _lib.current_stream()))
    return out


def heatmap_argmax(hm):
    """Device arg-max records of a heat-map tensor: cuda f32 [B,K,H,W] -> [B,K,6] (idx as int bits, max, l, r, u, d)."""
    import torch
    _lib.require_gpu()
    hm = hm.contiguous().float()
    B, K, H, W = hm.shape
    kp = torch.empty((B, K, 6), device=hm.device, dtype=torch.float32)
    _lib.check(_lib.lib().bp_heatmap_argmax(hm.data_ptr(), B, K, H, W, kp.data_ptr(), _lib.current_stream()))
    return kp
