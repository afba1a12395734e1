"""The fused per-frame path: frames resident in HBM -> 6D pose.

Device part (one hipGraph, ``bp_pipeline_run``): Pillow-exact bicubic stretch ->
YOLOv3 -> decode + arg-max objectness -> box rescale + crop -> FastPose -> heat-map
arg-max; 316 floats per frame come back.  Host part (``finish_record``): key-point
decoding, pPose-NMS (n = 1), key-point pruning, PnP.  Opt-in (``set_pose_solver``): the same
tail as one more launch at the end of the graph, 166 doubles per frame (``finish_pose_record``).  Together they replace
``DetectionLoader.update`` -> ``DetectionProcessor.update`` -> the KPD main loop ->
``DataWriter.update`` of the reference (dataloader.py:330-401,438-457,678-741;
betapose_evaluate.py:145-176) for the evaluation stream.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np

from . import _lib
from .eval import decode_keypoints
from .ops import solve_pnp, solve_pnp_ransac, solve_pnp_status
from .pPose_nms import pose_nms, pose_nms_picks

RESULT_FLOATS = _lib.RESULT_FLOATS
POSE_DOUBLES = _lib.POSE_DOUBLES
PNP_FAILED = "solve_pnp failed (need >= 6 non-degenerate points, or >= 4 coplanar ones)"   # bp_solve_pnp's error text


class _FrameChain:
    """What the three per-frame pipelines share -- the Python side of csrc/frame_chain.h.  A subclass names the prefix of
    its C entry points in ``_C``, creates ``frames`` and ``results`` and hands its handle to ``_open``."""
    _C = ""            # bp_pipeline / bp_scene / bp_cands
    _h = None
    poses = None       # torch f64 [rows, POSE_DOUBLES] once set_pose_solver was called

    def _fn(self, name: str):
        return getattr(_lib.lib(), "%s_%s" % (self._C, name))

    def _call(self, name: str, *args):
        _lib.check(self._fn(name)(self._h, *args))

    def _open(self, h):
        self._h = h
        self._run = self._fn("run")

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None:
                self._fn("destroy")(self._h)
                self._h = None
        except Exception:
            pass

    def _solver_args(self, kp3d, cam_K, rows: int):
        """(kp3d [n, 3], cam_K [3, 3]) as contiguous f64 arrays for the C call; ``self.poses`` [rows, 166] exists afterwards."""
        import torch
        k3 = np.ascontiguousarray(np.asarray(kp3d, dtype=np.float64).reshape(-1, 3))
        Kc = np.ascontiguousarray(np.asarray(cam_K, dtype=np.float64).reshape(3, 3))
        if self.poses is None:
            self.poses = torch.zeros((rows, POSE_DOUBLES), dtype=torch.float64, device=self.results.device)
            torch.cuda.current_stream(self.poses.device).synchronize()   # the fill is done before any stream writes rows
        return k3, Kc

    def enqueue(self, stream: Optional[int] = None):
        """Launch the device part on ``stream`` (default: torch's current stream).  ``self.frames`` must already hold the
        frame(s); ``self.results`` (and ``self.poses``) are valid once the stream reaches this point."""
        _lib.check(self._run(self._h, int(self.use_graph), stream if stream is not None else _lib.current_stream()))

    def prepare(self):
        """Set-up: build the frame's hipGraph now (capture + instantiate, nothing executes) instead of inside the first ``enqueue``."""
        if self.use_graph:
            self._call("prepare")
        return self

    def kernel_count(self) -> int:
        return self._fn("kernel_count")(self._h)

    def run(self, frames_bgr_u8) -> np.ndarray:
        """Convenience: upload the frame(s) (numpy [H,W,3] / [B,H,W,3] u8 or cuda tensor), run, return the records
        [rows,316] (host)."""
        import torch
        f = frames_bgr_u8 if hasattr(frames_bgr_u8, "is_cuda") else torch.from_numpy(np.ascontiguousarray(frames_bgr_u8))
        if f.dim() == 3:
            f = f.unsqueeze(0)
        self.frames.copy_(f, non_blocking=True)
        self.enqueue()
        return self.results.cpu().numpy()


class FramePipeline(_FrameChain):
    _C = "bp_pipeline"

    def __init__(self, det_model, pose_model, frame_h: int = 480, frame_w: int = 640, batch: int = 1,
                 confidence: float = 0.01, num_classes: int = 80, use_graph: bool = True, keep_heatmaps: bool = False,
                 frames=None):
        import torch
        _lib.require_gpu()
        self.det, self.pose = det_model, getattr(pose_model, "pyranet", pose_model)
        self.H, self.W, self.batch = int(frame_h), int(frame_w), int(batch)
        self.use_graph = bool(use_graph)
        self.det.cuda()
        self.pose.cuda()
        dev = "cuda:%d" % self.det._device
        # ``frames``: a device frame buffer shared with other pipelines (several objects looking at the same frame)
        self.frames = frames if frames is not None else torch.zeros((self.batch, self.H, self.W, 3), dtype=torch.uint8, device=dev)
        assert tuple(self.frames.shape) == (self.batch, self.H, self.W, 3) and self.frames.dtype == torch.uint8
        self.results = torch.zeros((self.batch, RESULT_FLOATS), dtype=torch.float32, device=dev)
        self.heatmaps = torch.zeros((self.batch, 50, 80, 64), dtype=torch.float32, device=dev) if keep_heatmaps else None
        h = C.c_void_p()
        _lib.check(_lib.lib().bp_pipeline_create(self.det.handle, self.pose.handle, self.H, self.W, self.batch,
                                                 float(confidence), int(num_classes), self.frames.data_ptr(),
                                                 self.results.data_ptr(),
                                                 self.heatmaps.data_ptr() if keep_heatmaps else None, C.byref(h)))
        self._open(h)
        self._faults_seen = 0

    def set_fixed_box(self, box_xyxy=None):
        """Throughput runs with a deterministic crop: box in frame pixels, or None."""
        if box_xyxy is None:
            self._call("set_fixed_box", None)
        else:
            b = np.ascontiguousarray(box_xyxy, dtype=np.float32)
            self._call("set_fixed_box", b.ctypes.data)

    def set_pose_solver(self, kp3d=None, cam_K=None, left_number: int = 50, ransac=None):
        """Opt-in device pose tail: every run then also writes ``self.poses`` [B, 166] f64, the frame's pose record
        (include/betapose_hip.h BP_POSE_DOUBLES; ``finish_pose_record`` turns it into ``finish_record``'s dict).
        ``kp3d`` [50, 3]: the 3-D key points; ``cam_K`` [3, 3]; ``left_number``: --left_keypoints.  None switches it off.
        ``ransac``: ``(reproj_err, max_trials, confidence)`` solves with the device RANSAC (``set_pose_ransac``) instead
        of the plain iterative PnP; None: the iterative tail."""
        if kp3d is None:
            self._call("set_pose_ransac", 0.0, 0, 0.0)
            self._call("set_pose_solver", None, 0, None, 0, None)
            return self
        k3, Kc = self._solver_args(kp3d, cam_K, self.batch)
        self._call("set_pose_solver", k3.ctypes.data, k3.shape[0], Kc.ctypes.data, int(left_number), self.poses.data_ptr())
        return self.set_pose_ransac(ransac)

    def set_pose_ransac(self, ransac=None):
        """``(reproj_err, max_trials, confidence)``: the device pose tail (which must be on) solves with RANSAC, the
        hypotheses in parallel (bp_pipeline_set_pose_ransac) -- the host solver's result, its inlier set in slot 15 of
        the pose row.  None (or ``max_trials`` 0): back to the iterative tail."""
        err, trials, conf = (0.0, 0, 0.0) if ransac is None else ransac
        self._call("set_pose_ransac", float(err), int(trials), float(conf))
        return self

    def enqueue(self, stream: Optional[int] = None):
        """Launch the device part on ``stream`` (default: torch's current stream).  ``self.frames`` must
        already hold the batch; ``self.results`` is valid once the stream reaches this point."""
        super().enqueue(stream)
        if any(getattr(m, "_latency_mode", False) for m in (self.det, self.pose)):
            self._latency_check()

    def latency_faults(self) -> int:
        """Frames this pipeline ran twice because the lone-frame latency mode's placement check failed (bp_pipeline_latency_faults)."""
        return int(_lib.lib().bp_pipeline_latency_faults(self._h))

    def _latency_check(self) -> bool:
        """Lone-frame latency mode only (Darknet.set_prefetch).  ``bp_pipeline_run`` itself waits for the frame in that mode, reads the
        engines' placement error words and -- when a launch reported a K slice on the wrong XCD, i.e. left a tile unstored -- switches
        the mode off and runs the same frame again, whichever caller drove it (``run``, ``StreamedRunner``, a bare ``enqueue``).  This
        mirrors that into the Python objects: a warning, and the engines' ``_latency_mode`` flags off (the mode stays off)."""
        n = self.latency_faults()
        if n == self._faults_seen:
            return False
        self._faults_seen = n
        import warnings
        warnings.warn("betapose_amd: block placement is not the round robin the lone-frame latency mode relies on; mode switched off, frame re-run")
        for m in (self.det, self.pose):
            if hasattr(m, "set_prefetch"):
                m.set_prefetch(False)
        return True


class ScenePipeline(_FrameChain):
    """A frame with several objects behind ONE multi-class detector pass (``bp_scene_*``): bicubic resize once, the shared
    detector once with the per-class select, then per object crop -> its key-point net -> arg-max -> (opt-in) its pose
    tail, all on one stream in one hipGraph.  ``pose_models``: {obj_id: FastPoseHIP}; ``class_of``: {obj_id: class id of
    the detector}.  ``results`` [K, 316] and ``poses`` [K, 166] hold one row per object in the order of ``obj_ids`` (the
    order of ``pose_models``); a row is the record ``FramePipeline`` writes for that object, select slots [6], [7] = class
    score, class id.  A class without a detection leaves index -1 in its row (``finish_record`` -> ``boxes`` None)."""
    _C = "bp_scene"

    def __init__(self, det_model, pose_models: dict, class_of: dict, frame_h: int = 480, frame_w: int = 640,
                 confidence: float = 0.01, num_classes: int = 80, use_graph: bool = True, frames=None):
        import torch
        from .darknet import check_class_ids
        self.obj_ids = list(pose_models)
        if not self.obj_ids:
            raise ValueError("ScenePipeline: no objects")
        missing = [o for o in self.obj_ids if o not in class_of]
        if missing:
            raise ValueError("ScenePipeline: no detector class for objects %s" % missing)
        self.class_ids = check_class_ids([class_of[o] for o in self.obj_ids], det_model.n_classes, num_classes)
        _lib.require_gpu()
        self.det = det_model
        self.poses_nets = [getattr(pose_models[o], "pyranet", pose_models[o]) for o in self.obj_ids]
        self.H, self.W, self.K = int(frame_h), int(frame_w), len(self.obj_ids)
        self.use_graph = bool(use_graph)
        self.det.cuda()
        for m in self.poses_nets:
            m.cuda()
        dev = "cuda:%d" % self.det._device
        self.frames = frames if frames is not None else torch.zeros((1, self.H, self.W, 3), dtype=torch.uint8, device=dev)
        assert tuple(self.frames.shape) == (1, self.H, self.W, 3) and self.frames.dtype == torch.uint8
        self.results = torch.zeros((self.K, RESULT_FLOATS), dtype=torch.float32, device=dev)
        kpds = (C.c_void_p * self.K)(*[m.handle for m in self.poses_nets])
        ids = (C.c_int * self.K)(*self.class_ids)
        h = C.c_void_p()
        _lib.check(_lib.lib().bp_scene_create(self.det.handle, C.cast(kpds, C.c_void_p), C.cast(ids, C.c_void_p), self.K, self.H,
                                              self.W, float(confidence), int(num_classes), self.frames.data_ptr(),
                                              self.results.data_ptr(), C.byref(h)))
        self._open(h)

    def set_pose_solver(self, obj_id, kp3d=None, cam_K=None, left_number: int = 50, ransac=None):
        """``FramePipeline.set_pose_solver`` for one object of the scene: its runs then also write row
        ``obj_ids.index(obj_id)`` of ``self.poses``.  ``kp3d`` None switches that object's tail off."""
        k = self.obj_ids.index(obj_id)
        if kp3d is None:
            self._call("set_pose_ransac", k, 0.0, 0, 0.0)
            self._call("set_pose_solver", k, None, 0, None, 0, None)
            return self
        k3, Kc = self._solver_args(kp3d, cam_K, self.K)
        self._call("set_pose_solver", k, k3.ctypes.data, k3.shape[0], Kc.ctypes.data, int(left_number),
                   self.poses.data_ptr() + k * POSE_DOUBLES * 8)
        err, trials, conf = (0.0, 0, 0.0) if ransac is None else ransac
        self._call("set_pose_ransac", k, float(err), int(trials), float(conf))
        return self


class CandidatePipeline(_FrameChain):
    """A frame through several NMS survivors of the detector (``bp_cands_*``): bicubic resize, the detector, the select
    with box NMS (``write_results``' NMS branch live, up to ``candidates`` boxes), ONE crop launch and ONE key-point pass
    at batch ``candidates``, arg-max, (opt-in) the candidate pose tail -- pPose-NMS merges the candidates' key points and
    the PnP runs on ``result[0]``.  ``results`` [C, 316] holds one ``FramePipeline`` record per candidate in survivor
    order, ``counts`` [1] their number; unused rows carry index -1.  ``pose_model`` needs ``max_batch >= candidates``.
    With ``candidates=1`` the row (and the pose row) is ``FramePipeline``'s, bit for bit."""
    _C = "bp_cands"

    def __init__(self, det_model, pose_model, frame_h: int = 480, frame_w: int = 640, candidates: int = 4,
                 nms_conf: float = 0.6, confidence: float = 0.01, num_classes: int = 80, class_id: int = 0,
                 use_graph: bool = True, frames=None):
        import torch
        Cn = int(candidates)
        if not 1 <= Cn <= _lib.MAX_CANDIDATES:
            raise ValueError("candidates must be 1 to %d, not %d" % (_lib.MAX_CANDIDATES, Cn))
        _lib.require_gpu()
        self.det, self.pose = det_model, getattr(pose_model, "pyranet", pose_model)
        self.H, self.W, self.C = int(frame_h), int(frame_w), Cn
        self.use_graph = bool(use_graph)
        self.det.cuda()
        self.pose.cuda()
        dev = "cuda:%d" % self.det._device
        self.frames = frames if frames is not None else torch.zeros((1, self.H, self.W, 3), dtype=torch.uint8, device=dev)
        assert tuple(self.frames.shape) == (1, self.H, self.W, 3) and self.frames.dtype == torch.uint8
        self.results = torch.zeros((Cn, RESULT_FLOATS), dtype=torch.float32, device=dev)
        self.merged = None         # torch f32 [C, MERGED_FLOATS]: device copies of the tail's merged poses ...
        self.info = None           # ... and int32 [4]: n, m, index of result[0], mask of the candidates merged into it
        self.inst_poses = None     # torch f64 [C, POSE_DOUBLES] with set_pose_solver(..., all_instances=True)
        h = C.c_void_p()
        _lib.check(_lib.lib().bp_cands_create(self.det.handle, self.pose.handle, Cn, self.H, self.W, float(confidence),
                                              int(num_classes), int(class_id), float(nms_conf), self.frames.data_ptr(),
                                              self.results.data_ptr(), C.byref(h)))
        self._open(h)
        self.counts = _device_view(_lib.lib().bp_cands_counts(self._h), (1,), torch.int32, self.results.device)

    def set_pose_solver(self, kp3d=None, cam_K=None, left_number: int = 50, all_instances: bool = False):
        """Opt-in candidate pose tail: every run then also writes ``self.poses`` [1, 166] f64 (``FramePipeline``'s pose
        record for ``result[0]``), ``self.merged`` [C, 152] and ``self.info`` [4]; ``finish_candidate_pose_record`` turns
        them into ``finish_candidate_records``' dict.  None switches it off.  (No RANSAC variant yet.)
        ``all_instances``: one more launch solves EVERY merged pose, not ``result[0]`` alone: ``self.inst_poses`` [C, 166]
        f64, row j the pose row of merged pose j (row 0 = ``self.poses[0]``, rows past the last merged pose status 1)."""
        import torch
        L = _lib.lib()
        if kp3d is None:
            self._call("set_pose_solver", None, 0, None, 0, None)
            self.inst_poses = None
            return self
        k3, Kc = self._solver_args(kp3d, cam_K, 1)
        self._call("set_pose_solver", k3.ctypes.data, k3.shape[0], Kc.ctypes.data, int(left_number), self.poses.data_ptr())
        dev = self.results.device
        self.merged = _device_view(L.bp_cands_merged(self._h), (self.C, _lib.MERGED_FLOATS), torch.float32, dev)
        self.info = _device_view(L.bp_cands_info(self._h), (4,), torch.int32, dev)
        if all_instances:
            if self.inst_poses is None:
                self.inst_poses = torch.zeros((self.C, POSE_DOUBLES), dtype=torch.float64, device=dev)
                torch.cuda.current_stream(dev).synchronize()
            self._call("set_instance_poses", 1, self.inst_poses.data_ptr())
        elif self.inst_poses is not None:
            self._call("set_instance_poses", 0, None)
            self.inst_poses = None
        return self

    def run(self, frame_bgr_u8):
        """Convenience: upload one frame (numpy [H,W,3] u8 or cuda tensor), run, return (rows [C,316], count) (host)."""
        return super().run(frame_bgr_u8), int(self.counts.cpu()[0])


# A frame's candidate results as ONE f32 row (StreamedRunner(candidates=C), the harness' gather): the pose row first (f64,
# so its offset stays 8-byte aligned), then the C records, the merged poses, the count and the info words (int bits);
# with ``instances`` the C instance pose rows (f64) follow everything else, after a pad word where they would otherwise
# start on an odd float.
def candidate_row_floats(C_: int, with_pose: bool, instances: bool = False) -> int:
    base = C_ * RESULT_FLOATS + 1 + ((2 * POSE_DOUBLES + C_ * _lib.MERGED_FLOATS + 4) if with_pose else 0)
    if not instances:
        return base
    if not with_pose:
        raise ValueError("instance rows need the pose tail (with_pose)")
    return base + (base & 1) + 2 * POSE_DOUBLES * C_


def _candidate_row_instances(row, C_: int):
    """View of the instance rows (f32 pairs, [2 * 166 * C]) at the end of a packed row that carries them."""
    base = candidate_row_floats(C_, True)
    a = base + (base & 1)
    return row[a:a + 2 * POSE_DOUBLES * C_]


def _candidate_row_parts(row, C_: int, with_pose: bool):
    """Views (pose f32-pairs, recs, merged, count, info) into a packed row (torch or numpy, f32 [W])."""
    a = 2 * POSE_DOUBLES if with_pose else 0
    b = a + C_ * RESULT_FLOATS
    c = b + (C_ * _lib.MERGED_FLOATS if with_pose else 0)
    return row[:a], row[a:b], row[b:c], row[c:c + 1], row[c + 1:c + 1 + (4 if with_pose else 0)]


def _pack_candidate_row(pinned, cp, with_pose: bool, instances: bool = False):
    import torch
    if instances:
        _candidate_row_instances(pinned, cp.C).view(torch.float64).view(cp.C, POSE_DOUBLES).copy_(cp.inst_poses, non_blocking=True)
    pose, recs, merged, count, info = _candidate_row_parts(pinned, cp.C, with_pose)
    recs.view(cp.C, RESULT_FLOATS).copy_(cp.results, non_blocking=True)
    count.view(torch.int32).copy_(cp.counts, non_blocking=True)
    if with_pose:
        pose.view(torch.float64).copy_(cp.poses[0], non_blocking=True)
        merged.view(cp.C, _lib.MERGED_FLOATS).copy_(cp.merged, non_blocking=True)
        info.view(torch.int32).copy_(cp.info, non_blocking=True)


def unpack_candidate_row(row, candidates: int, with_pose: bool, instances: bool = False):
    """A packed candidate row (numpy f32) -> (recs [C,316], count, pose_row [166] f64 or None, merged [C,152] or None,
    info [4] int32 or None); with ``instances`` a sixth value, the instance pose rows [C,166] f64."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    if instances:
        inst = np.ascontiguousarray(_candidate_row_instances(row, int(candidates))).view(np.float64)
        return unpack_candidate_row(row, candidates, with_pose) + (inst.reshape(int(candidates), POSE_DOUBLES),)
    pose, recs, merged, count, info = _candidate_row_parts(row, int(candidates), with_pose)
    n = int(count.view(np.int32)[0])
    recs = recs.reshape(int(candidates), RESULT_FLOATS)
    if not with_pose:
        return recs, n, None, None, None
    return (recs, n, np.ascontiguousarray(pose).view(np.float64), merged.reshape(int(candidates), _lib.MERGED_FLOATS),
            np.ascontiguousarray(info).view(np.int32))


def _device_view(ptr, shape, dtype, device):
    """A torch tensor over library-owned device memory (alive as long as the owning handle)."""
    import torch
    n = int(np.prod(shape))
    size = n * torch.empty((), dtype=dtype).element_size()

    class _Mem:
        __cuda_array_interface__ = {"shape": (size,), "typestr": "|u1", "data": (int(ptr), False), "version": 3}
    return torch.as_tensor(_Mem(), device=device).view(dtype).reshape(shape)


def frame_sharded_owner(n_objects: int, world: int):
    """Ownership of (frame, object) units when a shared detector serves all objects of a frame: the whole frame --
    units ``f * n_objects .. f * n_objects + n_objects - 1`` -- belongs to rank ``f % world``.  Returns ``owner(u)``."""
    K, world = int(n_objects), int(world)

    def owner(u: int) -> int:
        return (int(u) // K) % world
    return owner


def _copy_rows(rec, pose, pipe):
    rec.copy_(pipe.results, non_blocking=True)
    if pose is not None:
        pose.copy_(pipe.poses, non_blocking=True)


class _InflightRing:
    """The frames-in-flight machinery of the runners, and the only holder of it: ``S`` streams, ``2 S`` pinned record
    (and optional pose) slots with an event each, the queue of launches in flight, and the loader slots checked out of
    the source with the number of launches that still read each.  Launch j runs on stream ``j % S`` and lands in slot
    ``j % 2S``; the runner decides what a launch is and finishes the oldest one once the ring is ``full``.  Every index
    ``frames`` yields is released exactly once: by the ``finish`` of its last reader, by ``reads(idx, 0)``, or by ``abort``."""

    def __init__(self, device, S: int, rec_shape, pose_shape=None, copy_out=_copy_rows):
        """``rec_shape`` / ``pose_shape``: what one launch brings back (f32 rows / f64 pose rows or None);
        ``copy_out(rec_slot, pose_slot, pipe)`` queues the copies from ``pipe`` on the current stream."""
        import torch
        self.S = S
        self.streams = [torch.cuda.Stream(device=device) for _ in range(S)] if device is not None else []   # None: no engine, no launch
        self._pinned = [torch.empty(rec_shape, dtype=torch.float32).pin_memory() for _ in range(2 * S)]
        self._pinned_pose = [torch.empty(pose_shape, dtype=torch.float64).pin_memory() if pose_shape is not None else None
                             for _ in range(2 * S)]
        self._events = [torch.cuda.Event() for _ in range(2 * S)]
        self._copy_out = copy_out
        self._upload, self._on_stream = _lib.lib().bp_upload, torch.cuda.stream
        self.inflight = []         # (slot, tag, loader indices the launch reads), oldest first
        self.launched = 0          # j: launches submitted since ``frames`` began
        self.lane = 0              # j % S: the stream (and frame buffer) the next launch runs on
        self._out = {}             # loader index checked out -> launches that still read it
        self._source = None

    def frames(self, source):
        """Iterate ``source``; each ``(index, frame, host_address)`` is checked out, with one reader, as it is yielded."""
        self._source, self.launched, self.lane = source, 0, 0
        for item in source:
            self._out[item[0]] = 1
            yield item

    def reads(self, idx, launches: int):
        """``launches`` launches will read loader slot ``idx`` instead of one; 0 hands it back at once."""
        if launches:
            self._out[idx] = launches
        else:
            del self._out[idx]
            self._source.release(idx)

    @property
    def full(self) -> bool:
        return len(self.inflight) > self.S

    def upload(self, dst: int, addr: int, nbytes: int):
        """Host frame -> device address ``dst`` on the next launch's stream (which orders it behind that stream's previous launch)."""
        _lib.check(self._upload(dst, addr, nbytes, self.streams[self.lane].cuda_stream))

    def submit(self, pipe, tag, idxs):
        """Launch ``pipe`` on the lane's stream, copy its rows into the lane's pinned slot and record the slot's event.
        ``idxs``: the loader slots the launch reads; ``tag`` comes back from ``finish``."""
        st, slot = self.streams[self.lane], self.launched % len(self._events)
        with self._on_stream(st):
            pipe.enqueue(st.cuda_stream)
            self._copy_out(self._pinned[slot], self._pinned_pose[slot], pipe)
            self._events[slot].record(st)
        self.inflight.append((slot, tag, idxs))
        self.launched += 1
        self.lane = self.launched % self.S

    def finish(self):
        """Wait for the oldest launch -> ``(tag, rows, pose rows or None)`` (host copies); loader slots whose last reader
        it was are released first."""
        slot, tag, idxs = self.inflight.pop(0)
        self._events[slot].synchronize()
        recs = self._pinned[slot].numpy().copy()
        poses = self._pinned_pose[slot].numpy().copy() if self._pinned_pose[slot] is not None else None
        for idx in idxs:
            self._out[idx] -= 1
            if not self._out[idx]:
                del self._out[idx]
                self._source.release(idx)
        return tag, recs, poses

    def abort(self):
        """After an error mid-stream (a broken frame, a failed launch, a raising callback): let the device drain, then
        hand the loader every slot still checked out so it can be closed or iterated further."""
        if self.inflight or self._out:
            for st in self.streams:
                st.synchronize()
            for idx in list(self._out):
                try:
                    self._source.release(idx)
                except Exception:
                    pass
            self.inflight.clear()
            self._out.clear()


def _check_frame(idx, frame, H: int, W: int):
    if frame.shape != (H, W, 3):
        raise ValueError("frame %d is %s, pipeline was built for %s" % (idx, frame.shape, (H, W, 3)))


class StreamedRunner:
    """Keeps ``streams`` frames in flight: one engine clone + one hipGraph per HIP stream over shared filters, frame
    uploads straight from the loader's pinned slots, records copied back into a ring of pinned buffers.  At batch 1
    most layers cannot fill 256 CUs and every kernel carries a few microseconds of fixed cost, so independent frames
    overlapping on the chip is where the throughput comes from."""

    def __init__(self, det_model, pose_model, frame_h: int = 480, frame_w: int = 640, streams: int = 4,
                 confidence: float = 0.01, num_classes: int = 80, use_graph: bool = True, batch: int = 1,
                 pose_solver=None, candidates: Optional[int] = None, nms_conf: float = 0.6, all_instances: bool = False):
        """``all_instances`` (with ``candidates`` and a ``pose_solver``): every stream's tail solves every merged pose and
        the packed row carries the instance rows (``unpack_candidate_row(..., instances=True)``).
        ``candidates`` = C: every stream owns one ``CandidatePipeline`` (up to C NMS survivors per frame at box-NMS
        threshold ``nms_conf``, one frame per launch; ``pose_model`` needs ``max_batch >= C``) and ``on_record`` gets
        ``(index, row)`` with the frame's packed candidate row (``unpack_candidate_row``); ``pose_solver`` is then
        ``(kp3d, cam_K, left_number)`` -- the candidate tail has no RANSAC variant.
        ``pose_solver``: ``(kp3d, cam_K, left_number)`` or ``(kp3d, cam_K, left_number, ransac)`` turns the device pose tail on in every stream's pipeline; the
        pose rows then come back with the records and ``on_record`` gets ``(index, rec, pose_row)``.
        ``batch`` frames per launch and stream (the reference's ``--detbatch``, dataloader.py:284-289): the engines
        must have been created with ``max_batch >= batch``.  More frames per launch mean fewer launches, K slices and
        hand-offs per frame: 1 -> 2 -> 4 frames per launch run 945 -> 1 100 -> 1 290 frames/s."""
        S = max(1, int(streams))
        B = max(1, int(batch))
        pose = getattr(pose_model, "pyranet", pose_model)
        dets = [det_model] + [det_model.clone() for _ in range(S - 1)]
        poses = [pose] + [pose.clone() for _ in range(S - 1)]
        self.C = None if candidates is None else int(candidates)
        instances = bool(all_instances)
        if instances and (self.C is None or pose_solver is None):
            raise ValueError("StreamedRunner: all_instances needs candidates=C and a pose_solver")
        self.B, self.H, self.W = B, int(frame_h), int(frame_w)
        with_pose = pose_solver is not None
        if self.C is not None:
            if B != 1:
                raise ValueError("StreamedRunner: candidates run one frame per launch (batch=1), not batch=%d" % B)
            if with_pose and len(pose_solver) > 3 and pose_solver[3] is not None:
                raise ValueError("StreamedRunner: the candidate pose tail has no RANSAC variant")
            self.pipes = [CandidatePipeline(dets[k], poses[k], frame_h, frame_w, candidates=self.C, nms_conf=nms_conf,
                                            confidence=confidence, num_classes=num_classes, use_graph=use_graph) for k in range(S)]
            if with_pose:
                for cp in self.pipes:
                    cp.set_pose_solver(*pose_solver[:3], all_instances=instances)
            self._ring = _InflightRing(self.pipes[0].frames.device, S, (candidate_row_floats(self.C, with_pose, instances),),
                                       copy_out=lambda row, _, cp: _pack_candidate_row(row, cp, with_pose, instances))
            return
        self.pipes = [FramePipeline(dets[k], poses[k], frame_h, frame_w, batch=B, confidence=confidence,
                                    num_classes=num_classes, use_graph=use_graph) for k in range(S)]
        if with_pose:
            for fp in self.pipes:
                fp.set_pose_solver(*pose_solver)
        self._ring = _InflightRing(self.pipes[0].frames.device, S, (B, RESULT_FLOATS), (B, POSE_DOUBLES) if with_pose else None)

    def run(self, source, on_record) -> int:
        """``source`` yields ``(index, frame[H,W,3] u8 BGR, host_address)`` and has ``release(index)`` (FrameLoader);
        ``on_record(index, rec[316])`` -- ``(index, rec[316], pose_row[166])`` with a pose solver -- is called in source
        order once the frame's record is on the host.
        Returns the number of frames processed."""
        ring, B, nbytes = self._ring, self.B, self.H * self.W * 3
        pending = []           # source indices uploaded into the current launch's batch slots

        def launch():
            idxs = tuple(pending)
            pending.clear()
            ring.submit(self.pipes[ring.lane], idxs, idxs)

        def deliver():
            idxs, recs, poses = ring.finish()
            if self.C is not None:
                on_record(idxs[0], recs)
                return
            for b, idx in enumerate(idxs):
                if poses is None:
                    on_record(idx, recs[b])
                else:
                    on_record(idx, recs[b], poses[b])

        n = 0
        try:
            for idx, frame, addr in ring.frames(source):
                _check_frame(idx, frame, self.H, self.W)
                ring.upload(self.pipes[ring.lane].frames.data_ptr() + len(pending) * nbytes, addr, nbytes)
                pending.append(idx)
                n += 1
                if len(pending) == B:
                    launch()
                    if ring.full:              # (the stream's own order keeps a launch's frame slots safe from the next upload)
                        deliver()
            if pending:                        # ragged last launch: the unused slots keep their previous frames, whose
                launch()                       # records nobody reads
            while ring.inflight:
                deliver()
        except BaseException:
            ring.abort()
            raise
        return n


class MultiObjectRunner:
    """Occlusion-LineMod as a multi-object workload (occlusion_betapose_evaluate.py:89-90,204,218-257 runs ONE object
    per process and re-decodes every frame per object): the unit of work is a (frame, object) pair.  Every
    object keeps its own detector + key-point weights resident; a frame is decoded ONCE (loader slot), and each of its
    units uploads it from that slot to the stream it lands on and runs that object's graph.  ``streams`` units are in
    flight; unit u = frame_position * n_objects + object_position, and only the units in ``owned`` are run (the caller
    shards them ``u % world``).

    ``engines``: {obj_id: (Darknet, FastPoseHIP)} for the objects this rank owns units of.  ``pose_solvers``:
    {obj_id: (kp3d, cam_K, left_number[, ransac])} turns the device pose tail on (every object in ``engines`` needs one); then
    ``on_record`` gets ``(u, rec, pose_row)``.

    ``shared_detector``: ``(Darknet, {obj_id: class id})`` -- one multi-class detector serves every object.  ``engines``
    is then {obj_id: FastPoseHIP} for ALL of ``obj_ids``, each stream owns one ``ScenePipeline`` (clones over shared
    filters), and the unit of scheduling is the frame: the K units of a frame run in one graph on one stream, so
    ``owned`` must give a frame's units to one rank (``frame_sharded_owner``).  ``on_record`` is still called once per
    unit, with that object's row."""

    def __init__(self, engines: dict, obj_ids: List[int], frame_h: int = 480, frame_w: int = 640, streams: int = 4,
                 confidence: float = 0.01, num_classes: int = 80, use_graph: bool = True, pose_solvers: Optional[dict] = None,
                 shared_detector=None):
        self.obj_ids = list(obj_ids)
        S = max(1, int(streams))
        self.H, self.W = int(frame_h), int(frame_w)
        self.pipes = {}            # (stream, obj_id) -> FramePipeline over the stream's shared frame buffer
        self.scenes = None         # shared_detector: one ScenePipeline per stream
        self.frame_bufs = []
        rows = 1                   # rows a launch brings back: one unit, or a frame's K behind the shared detector
        if shared_detector is not None:
            det, class_of = shared_detector
            missing = [o for o in self.obj_ids if o not in engines]
            if missing:
                raise ValueError("shared detector: no key-point engine for objects %s" % missing)
            rows = len(self.obj_ids)
            self.scenes = []
            for k in range(S):
                poses = {o: getattr(engines[o], "pyranet", engines[o]) for o in self.obj_ids}
                d = det if k == 0 else det.clone()
                if k:
                    poses = {o: m.clone() for o, m in poses.items()}
                sp = ScenePipeline(d, poses, class_of, frame_h, frame_w, confidence=confidence, num_classes=num_classes,
                                   use_graph=use_graph)
                if pose_solvers is not None:
                    for o in self.obj_ids:
                        sp.set_pose_solver(o, *pose_solvers[o])
                self.scenes.append(sp)
                self.frame_bufs.append(sp.frames)
        else:
            for k in range(S):
                buf = None
                for oid, (det, pose) in engines.items():
                    pose = getattr(pose, "pyranet", pose)
                    d, p_ = (det, pose) if k == 0 else (det.clone(), pose.clone())
                    fp = FramePipeline(d, p_, frame_h, frame_w, batch=1, confidence=confidence, num_classes=num_classes,
                                       use_graph=use_graph, frames=buf)
                    if pose_solvers is not None:
                        fp.set_pose_solver(*pose_solvers[oid])
                    buf = fp.frames
                    self.pipes[(k, oid)] = fp
                self.frame_bufs.append(buf)
        dev = self.frame_bufs[0].device if self.frame_bufs[0] is not None else None
        self._ring = _InflightRing(dev, S, (rows, RESULT_FLOATS), (rows, POSE_DOUBLES) if pose_solvers is not None else None)

    def run(self, source, frame_positions: List[int], owned, on_record) -> int:
        """``source``: FrameLoader over the frames this rank touches (in ``frame_positions`` order: position of each
        in the global frame list); ``owned(u)`` tells whether unit u belongs to this rank;
        ``on_record(u, rec[316])`` receives every owned unit's record.  Returns the number of units run.
        Behind a shared detector a frame is the unit in flight (``streams`` of them): its K rows come back together and
        are handed out unit by unit."""
        ring, nbytes, K, shared = self._ring, self.H * self.W * 3, len(self.obj_ids), self.scenes is not None

        def deliver():
            u, recs, poses = ring.finish()     # u: the launch's first unit, one row per unit
            for r in range(len(recs)):
                if poses is None:
                    on_record(u + r, recs[r])
                else:
                    on_record(u + r, recs[r], poses[r])

        try:
            for idx, frame, addr in ring.frames(source):
                _check_frame(idx, frame, self.H, self.W)
                f = frame_positions[idx]
                units = [u for u in range(f * K, f * K + K) if owned(u)]
                if shared and units:
                    if len(units) < K:
                        raise ValueError("shared detector: the units of frame %d are split over ranks (shard by frame)" % f)
                    units = units[:1]
                ring.reads(idx, len(units))    # nobody's frame: released at once without a launch
                for u in units:
                    # the stream's frame buffer is only rewritten after the stream's previous unit finished reading it
                    # (same stream: in order)
                    k = ring.lane
                    ring.upload(self.frame_bufs[k].data_ptr(), addr, nbytes)
                    ring.submit(self.scenes[k] if shared else self.pipes[(k, self.obj_ids[u % K])], u, (idx,))
                    if ring.full:
                        deliver()
            while ring.inflight:
                deliver()
        except BaseException:
            ring.abort()
            raise
        return ring.launched * (K if shared else 1)


def finish_record(rec: np.ndarray, imgname: str, kp_3d: np.ndarray, cam_K: np.ndarray, left_number: int = 50,
                  ransac=None) -> dict:
    """Host tail for one frame: 316-float record -> the dict ``DataWriter.update`` appends to
    ``final_result`` (dataloader.py:704-727): {'imgname', 'result', 'cam_R', 'cam_t'} (+ the raw boxes).
    ``ransac``: ``(reproj_err, max_trials, confidence)`` solves the pruned points with ``ops.solve_pnp_ransac`` (the
    variant utils/utils.py:32-36 keeps commented out) and adds 'pnp_inliers', a bool array over the kept points."""
    rec = np.ascontiguousarray(rec, dtype=np.float32)
    idx = int(rec[:1].view(np.int32)[0])
    if idx < 0:     # no detection: the reference forwards the frame with boxes=None and records nothing
        return {"imgname": imgname, "result": [], "cam_R": [], "cam_t": [], "boxes": None}
    boxes = rec[12:16].reshape(1, 4).copy()
    scores = rec[5:6].reshape(1, 1).copy()
    pt1, pt2 = rec[8:10].reshape(1, 2), rec[10:12].reshape(1, 2)
    kp = rec[16:].reshape(1, 50, 6)
    _, preds_img, preds_scores = decode_keypoints(kp, pt1, pt2)
    result = pose_nms(boxes, scores, preds_img, preds_scores)
    out = {"imgname": imgname, "result": result, "boxes": boxes, "scores": scores, "yolo_index": idx}
    if result:
        kp_score = np.array(result[0]["kp_score"][:, 0])
        kp_2d = np.array(result[0]["keypoints"])
        k3 = np.array(kp_3d)
        while len(kp_2d) > left_number:          # dataloader.py:718-722
            d = int(np.argmin(kp_score, axis=0))
            kp_score = np.delete(kp_score, d)
            kp_2d = np.delete(kp_2d, d, axis=0)
            k3 = np.delete(k3, d, axis=0)
        if ransac is not None:
            R, t, inl = solve_pnp_ransac(k3, kp_2d, cam_K, ransac[0], ransac[1], ransac[2])
            out["pnp_inliers"] = inl
        else:
            R, t = solve_pnp(k3, kp_2d, cam_K)
        out.update({"cam_R": R, "cam_t": t})
    else:
        out.update({"cam_R": [], "cam_t": []})
    return out


def _prune_keypoints(human: dict, kp_3d: np.ndarray, left_number: int):
    """dataloader.py:718-722 on one merged pose: drop the lowest score until ``left_number`` remain -> (kp_3d, kp_2d)."""
    kp_score = np.array(human["kp_score"][:, 0])
    kp_2d = np.array(human["keypoints"])
    k3 = np.array(kp_3d)
    while len(kp_2d) > left_number:
        d = int(np.argmin(kp_score, axis=0))
        kp_score = np.delete(kp_score, d)
        kp_2d = np.delete(kp_2d, d, axis=0)
        k3 = np.delete(k3, d, axis=0)
    return k3, kp_2d


def _host_instances(out: dict, picks, kp_3d: np.ndarray, cam_K: np.ndarray, left_number: int) -> list:
    """The ``"instances"`` list for a host dict whose ``result[0]`` is already solved: entry 0 carries the frame's pose,
    every other merged pose goes through the same pruning and ``solve_pnp``; its failure is recorded, not raised."""
    inst = []
    for j, human in enumerate(out["result"]):
        pk = int(picks[j])
        if j == 0:
            R, t, st = out["cam_R"], out["cam_t"], 0
            npts = min(len(human["keypoints"]), max(int(left_number), 0))
        else:
            k3, kp_2d = _prune_keypoints(human, kp_3d, left_number)
            R, t, st = solve_pnp_status(k3, kp_2d, cam_K)
            npts = len(kp_2d)
        inst.append({"cam_R": R, "cam_t": t, "status": st, "points": npts, "pick": pk, "bbox": out["boxes"][pk].copy()})
    return inst


def finish_candidate_records(recs: np.ndarray, count: int, imgname: str, kp_3d: np.ndarray, cam_K: np.ndarray,
                             left_number: int = 50, all_instances: bool = False) -> dict:
    """Host tail over the frame's ``count`` candidates (``CandidatePipeline`` rows [C, 316]): every candidate's key
    points are decoded, ``pose_nms`` clusters and merges them (pPose_nms.py:24-122 with n rows, what ``DataWriter.update``
    does with several boxes), and the PnP runs on ``result[0]`` after the ``left_number`` pruning.  With ``count`` 1 it is
    ``finish_record``'s dict.
    ``all_instances``: the dict gains ``"instances"``, a list parallel to ``"result"``: {"cam_R", "cam_t", "status",
    "points", "pick", "bbox"} per merged pose -- its own pruned PnP (entry 0: the frame's ``cam_R`` / ``cam_t``), the
    solver's code and the points it used, the candidate the pose was built around and that candidate's box
    (``result[j]["bbox"]`` stays the first box, pPose_nms.py:116).  A failed PnP of an entry j > 0 is recorded (empty
    ``cam_R`` / ``cam_t``, ``status`` < 0), not raised."""
    recs = np.ascontiguousarray(recs, dtype=np.float32).reshape(-1, RESULT_FLOATS)
    n = int(count)
    if n <= 0:
        out = {"imgname": imgname, "result": [], "cam_R": [], "cam_t": [], "boxes": None}
        if all_instances:
            out["instances"] = []
        return out
    if n == 1:
        out = finish_record(recs[0], imgname, kp_3d, cam_K, left_number)
        if all_instances:
            out["instances"] = _host_instances(out, [0] * len(out["result"]), kp_3d, cam_K, left_number)
        return out
    recs = recs[:n]
    idx = recs[:, :1].copy().view(np.int32)[:, 0]
    boxes = recs[:, 12:16].copy()
    scores = recs[:, 5:6].copy()
    kp = recs[:, 16:].reshape(n, 50, 6)
    _, preds_img, preds_scores = decode_keypoints(kp, recs[:, 8:10], recs[:, 10:12])
    result, picks = pose_nms_picks(boxes, scores, preds_img, preds_scores)
    out = {"imgname": imgname, "result": result, "boxes": boxes, "scores": scores, "yolo_index": int(idx[0]),
           "yolo_indices": idx}
    if result:
        k3, kp_2d = _prune_keypoints(result[0], kp_3d, left_number)
        R, t = solve_pnp(k3, kp_2d, cam_K)
        out.update({"cam_R": R, "cam_t": t})
    else:
        out.update({"cam_R": [], "cam_t": []})
    if all_instances:
        out["instances"] = _host_instances(out, picks, kp_3d, cam_K, left_number)
    return out


def _device_instances(out: dict, picks, inst_poses: np.ndarray) -> list:
    """The ``"instances"`` list from the device's instance rows [C, 166]: ``_host_instances``' entries, nothing redone."""
    rows = np.asarray(inst_poses, dtype=np.float64).reshape(-1, POSE_DOUBLES)
    inst = []
    for j in range(len(out["result"])):
        r = rows[j]
        st, pk = int(r[0]), int(picks[j])
        if j == 0:
            R, t = out["cam_R"], out["cam_t"]
        elif st == 0:
            R, t = r[2:11].reshape(3, 3).copy(), r[11:14].reshape(3, 1).copy()
        else:
            R, t = [], []
        inst.append({"cam_R": R, "cam_t": t, "status": st, "points": int(r[1]), "pick": pk, "bbox": out["boxes"][pk].copy()})
    return inst


def finish_candidate_pose_record(recs: np.ndarray, count: int, pose_row: np.ndarray, merged: np.ndarray, info: np.ndarray,
                                 imgname: str, inst_poses: Optional[np.ndarray] = None) -> dict:
    """Device-tail twin of ``finish_candidate_records``: the rows [C, 316], their count, the pose row [166], the merged
    poses [C, 152] and the info words [4] of the candidate pose tail -> the same dict, no arithmetic redone.
    ``inst_poses`` [C, 166] (``CandidatePipeline.inst_poses``): the dict of ``all_instances=True``."""
    recs = np.ascontiguousarray(recs, dtype=np.float32).reshape(-1, RESULT_FLOATS)
    n = int(count)
    info = np.asarray(info, dtype=np.int32).reshape(4)
    if n == 1:
        out = finish_pose_record(recs[0], pose_row, imgname)
        if inst_poses is not None:
            out["instances"] = _device_instances(out, [0] * len(out["result"]), inst_poses)
        return out
    row = np.asarray(pose_row, dtype=np.float64).reshape(POSE_DOUBLES)
    status = int(row[0])
    if (n <= 0) != (status == 1) or (n > 0 and int(info[0]) != n):
        raise ValueError("pose record (status %d, %d candidates) does not belong to these %d candidate records" % (status, int(info[0]), n))
    if n <= 0:
        out = {"imgname": imgname, "result": [], "cam_R": [], "cam_t": [], "boxes": None}
        if inst_poses is not None:
            out["instances"] = []
        return out
    if status < 0:
        raise _lib.BetaposeHipError(PNP_FAILED)
    recs = recs[:n]
    idx = recs[:, :1].copy().view(np.int32)[:, 0]
    boxes = recs[:, 12:16].copy()
    scores = recs[:, 5:6].copy()
    mg = np.ascontiguousarray(merged, dtype=np.float32).reshape(-1, _lib.MERGED_FLOATS)
    out = {"imgname": imgname, "boxes": boxes, "scores": scores, "yolo_index": int(idx[0]), "yolo_indices": idx}
    result = []
    for j in range(int(info[1])):
        kp = mg[j, 2:].reshape(50, 3)
        result.append({"bbox": boxes[0].copy(),                          # always the first box (pPose_nms.py:116)
                       "keypoints": kp[:, :2].copy(),
                       "kp_score": kp[:, 2:3].copy(),
                       "proposal_score": mg[j, 1:2].copy()})
    out["result"] = result
    if status == 2:
        out.update({"cam_R": [], "cam_t": []})
    else:
        out.update({"cam_R": row[2:11].reshape(3, 3).copy(), "cam_t": row[11:14].reshape(3, 1).copy()})
    if inst_poses is not None:
        out["instances"] = _device_instances(out, mg[:len(result), :1].copy().view(np.int32)[:, 0], inst_poses)
    return out


def finish_pose_record(rec: np.ndarray, pose_row: np.ndarray, imgname: str) -> dict:
    """Device-tail twin of ``finish_record``: the frame's 316-float record and its 166-double pose record (device pose
    tail, ``FramePipeline.set_pose_solver`` / ``bp_pose_from_records``) -> the same dict ``finish_record`` returns for
    the solver's kp3d / cam_K / left_number.  Raises ``BetaposeHipError`` where the host path raises."""
    rec = np.ascontiguousarray(rec, dtype=np.float32)
    row = np.asarray(pose_row, dtype=np.float64).reshape(POSE_DOUBLES)
    idx = int(rec[:1].view(np.int32)[0])
    status = int(row[0])
    if (idx < 0) != (status == 1):
        raise ValueError("pose record (status %d) does not belong to this frame record (index %d)" % (status, idx))
    if idx < 0:
        return {"imgname": imgname, "result": [], "cam_R": [], "cam_t": [], "boxes": None}
    if status < 0:
        raise _lib.BetaposeHipError(PNP_FAILED)
    boxes = rec[12:16].reshape(1, 4).copy()
    scores = rec[5:6].reshape(1, 1).copy()
    out = {"imgname": imgname, "boxes": boxes, "scores": scores, "yolo_index": idx}
    if status == 2:
        out.update({"result": [], "cam_R": [], "cam_t": []})
        return out
    kp = row[16:].reshape(50, 3).astype(np.float32)
    out["result"] = [{"bbox": boxes[0].copy(),
                      "keypoints": kp[:, :2].copy(),
                      "kp_score": kp[:, 2:3].copy(),
                      "proposal_score": np.array([row[14]], dtype=np.float32)}]
    if row[15] != 0:      # RANSAC tail: bit j of the integer-valued slot is the j-th point handed to the PnP
        out["pnp_inliers"] = ((int(row[15]) >> np.arange(int(row[1]), dtype=np.int64)) & 1).astype(bool)
    out.update({"cam_R": row[2:11].reshape(3, 3).copy(), "cam_t": row[11:14].reshape(3, 1).copy()})
    return out
