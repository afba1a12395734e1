"""Key-point annotation (stage 2 of the reference, ``2_keypoint_annotator/annotate_keypoint.py``) and the heat-map targets
its consumer draws from the annotations (``train_KPD/src/utils/pose.py`` generateSampleBox).

The wrappers follow metrics.render_depth: ``device=None`` runs the host twin of libbetapose_hip.so (no GPU needed), a
torch device the kernels of csrc/annotate.hip; the two agree bit for bit.  Definitions: DESIGN.md 3.8.
"""
from __future__ import annotations

import os

import numpy as np

from .metrics import BOP_VSD_DELTA, _poses34, render_depth

FRONT, IN_IMAGE, SELF_VISIBLE, SCENE_VISIBLE, SCENE_KNOWN = 1, 2, 4, 8, 16
VISIBLE = FRONT | IN_IMAGE | SELF_VISIBLE | SCENE_VISIBLE      # a key point a camera at the pose sees


def _size(size):
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1 or H * W > 1 << 24:
        raise ValueError("size = (H, W) must be positive with H * W <= 2^24")
    return H, W


def _K9(K):
    K = np.ascontiguousarray(K, dtype=np.float64)
    if K.size != 9:
        raise ValueError("K must be 3x3")
    return K.reshape(9)


def _scene_args(scene_depth, scene_index, P, H, W):
    """(scene [T, H, W] float32 or None, index [P] int32 or None, T), checked."""
    if scene_depth is None:
        if scene_index is not None:
            raise ValueError("scene_index without scene_depth")
        return None, None, 0
    scene = np.ascontiguousarray(scene_depth)
    if scene.dtype != np.float32 or scene.ndim != 3 or scene.shape[1:] != (H, W):
        raise ValueError("scene_depth must be a float32 array [T, %d, %d] (scene_depth_from_u16)" % (H, W))
    if scene_index is None:
        if len(scene) != P:
            raise ValueError("scene_index is needed unless scene_depth holds one image per pose")
        scene_index = np.arange(P)
    idx = np.ascontiguousarray(scene_index, dtype=np.int32).reshape(-1)
    if len(idx) != P:
        raise ValueError("scene_index needs one entry per pose")
    if P and (idx.min() < 0 or idx.max() >= len(scene)):
        raise ValueError("a scene index lies outside [0, %d)" % len(scene))
    return scene, idx, len(scene)


def _depth_stack(depth, H=None, W=None, P=None, name="depth"):
    d = np.ascontiguousarray(depth)
    if d.dtype != np.float32 or d.ndim != 3:
        raise ValueError("%s must be a float32 array [P, H, W]" % name)
    if (H is not None and d.shape[1:] != (H, W)) or (P is not None and len(d) != P):
        raise ValueError("%s has shape %s, expected (%s, %s, %s)" % (name, d.shape, P, H, W))
    return d


def scene_depth_from_u16(frames_u16, depth_scale):
    """Test depth images [T, H, W] uint16 -> float32 in pose units, ``raw.astype(float64) * depth_scale`` cast to
    float32: the one conversion both the host and the device path of this module read (0 stays 0 = missing)."""
    raw = np.asarray(frames_u16)
    if raw.dtype != np.uint16:
        raise ValueError("frames_u16 must be uint16")
    return np.ascontiguousarray((raw.astype(np.float64) * float(depth_scale)).astype(np.float32))


def project_keypoints(poses, kp3d, K, size, model_depth=None, scene_depth=None, scene_index=None, self_tol=BOP_VSD_DELTA,
                      delta=BOP_VSD_DELTA, pixel_center=0.0, near=0.01, device=None):
    """Labels of ``Kp`` model points at ``P`` poses: ``(xy [P, Kp, 2] float64, z [P, Kp] float64, flags [P, Kp] uint8)``.
    ``xy`` is the projection ``((fx X + s Y) / Z + cx, fy Y / Z + cy)`` of ``X = R m + t`` (the reference's project_kp
    order), ``z`` its camera depth.  Flag bits: FRONT (``Z >= near``), IN_IMAGE (the pixel
    ``floor(xy - pixel_center + 0.5)`` exists in ``size = (H, W)``), SELF_VISIBLE (the pose's own render
    ``model_depth[p]``, render_depth's output for the same poses and pixel_center, does not cover that pixel with a
    depth below ``Z - self_tol``), SCENE_VISIBLE (the scene depth ``S`` there, image ``scene_index[p]`` of
    ``scene_depth`` [T, H, W] float32 in pose units, is 0 = missing or ``Z - S <= delta``) and SCENE_KNOWN (``S > 0``).
    A depth input that is not given leaves its bit set for every FRONT and IN_IMAGE point; a point that is not FRONT
    has ``xy = (-1, -1)`` and flags 0."""
    from . import _lib
    poses = _poses34(poses)
    kp = np.ascontiguousarray(kp3d, dtype=np.float64).reshape(-1, 3)
    H, W = _size(size)
    Kf = _K9(K)
    P, Kp = len(poses), len(kp)
    if Kp < 1:
        raise ValueError("at least one key point")
    if not near > 0:
        raise ValueError("near must be positive")
    md = None if model_depth is None else _depth_stack(model_depth, H, W, P, "model_depth")
    scene, idx, T = _scene_args(scene_depth, scene_index, P, H, W)
    if P == 0:
        return np.empty((P, Kp, 2), np.float64), np.empty((P, Kp), np.float64), np.empty((P, Kp), np.uint8)
    side = _lib.Side(device)
    xy, z, flags = side.empty((P, Kp, 2), np.float64), side.empty((P, Kp), np.float64), side.empty((P, Kp), np.uint8)
    side.call("bp_annotate_keypoints", side.put(poses), P, side.put(kp), Kp, _lib.ptr(Kf), H, W, float(pixel_center), float(near),
              side.put(md), side.put(scene), T, side.put(idx), float(self_tol), float(delta), xy, z, flags)
    return side.get(xy), side.get(z), side.get(flags)


def mask_boxes(depth, K, scene_depth=None, scene_index=None, delta=BOP_VSD_DELTA, pixel_center=0.0, device=None):
    """Boxes of ``P`` depth images [P, H, W] float32 (render_depth's): ``(boxes [P, 2, 4] int32, counts [P, 2] int32)``.
    Box 0 surrounds the covered pixels (depth > 0), box 1 those of them that metrics.vsd_masks calls ``visib_gt``
    against the scene depth (distances along the pixel's ray, ``delta``, missing scene depth counts as visible); both
    are the reference's get_bbox_from_mask order ``(xmin, xmax, ymin, ymax)``, inclusive, and ``-1`` four times when
    empty.  ``counts`` are the two pixel counts, so ``counts[:, 1] / counts[:, 0]`` is BOP's ``visib_fract``.  Without a
    scene depth box 1 equals box 0."""
    from . import _lib
    d = _depth_stack(depth)
    P, H, W = d.shape
    _size((H, W))
    Kf = _K9(K)
    scene, idx, T = _scene_args(scene_depth, scene_index, P, H, W)
    if P == 0:
        return np.empty((P, 2, 4), np.int32), np.empty((P, 2), np.int32)
    side = _lib.Side(device)
    boxes, counts = side.empty((P, 2, 4), np.int32), side.empty((P, 2), np.int32)
    side.call("bp_mask_boxes", side.put(d), P, H, W, _lib.ptr(Kf), float(pixel_center), side.put(scene), T, side.put(idx),
              float(delta), boxes, counts)
    return side.get(boxes), side.get(counts)


def vertex_boxes(poses, vertices, K, size, device=None):
    """The reference's ``mask_bbox`` (sinobj.project_all) of ``P`` poses: every vertex is splatted into the pixel
    ``(int(x), int(y))`` of its projection, truncated toward zero, and the box ``(xmin, xmax, ymin, ymax)`` is taken over
    the vertices with ``0 < int(x) < W`` and ``0 < int(y) < H`` (the reference's strict bounds); ``-1`` four times
    when none qualifies.  int32 [P, 4]."""
    from . import _lib
    poses = _poses34(poses)
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    H, W = _size(size)
    Kf = _K9(K)
    P = len(poses)
    if len(v) < 1:
        raise ValueError("at least one vertex")
    if P == 0:
        return np.empty((P, 4), np.int32)
    side = _lib.Side(device)
    boxes = side.empty((P, 4), np.int32)
    side.call("bp_vertex_boxes", side.put(poses), P, side.put(v), len(v), _lib.ptr(Kf), H, W, boxes)
    return side.get(boxes)


def gaussian_table(sigma=1):
    """drawGaussian's patch (train_KPD/src/utils/img.py:74-80) for ``hmGauss = sigma``: its numpy expression, cast to
    float32 as the assignment into the float32 map casts it.  [6 sigma + 1, 6 sigma + 1]."""
    sigma = int(sigma)
    if sigma < 1:
        raise ValueError("sigma must be a positive integer")
    tmpSize = 3 * sigma
    size = 2 * tmpSize + 1
    x = np.arange(0, size, 1, float)
    y = x[:, np.newaxis]
    x0 = y0 = size // 2
    sigma = size / 4.0
    g = np.exp(- ((x - x0) ** 2 + (y - y0) ** 2) / (2 * sigma ** 2))
    return np.ascontiguousarray(g.astype(np.float32))


def kpd_targets(parts, ul, br, in_res=(320, 256), out_res=(80, 64), sigma=1, want_mask=False, device=None, as_tensor=False):
    """The label half of generateSampleBox ('coco' branch) for ``B`` samples: ``parts`` [B, Kp, 2] float64 image
    coordinates and the windows ``ul``, ``br`` [B, 2] float32 (kpd_windows) give ``(out [B, Kp, resH, resW] float32,
    centres [B, Kp, 2] int32)``, and ``setMask`` (all ones, as the reference returns it) as a third with ``want_mask``.
    A part is drawn iff ``x > 0`` and it lies strictly inside its window; its centre is transformBox's (float32
    arithmetic, round half to even), its patch drawGaussian's clipped copy of gaussian_table(sigma); an undrawn part
    has centre ``(-1, -1)`` and a zero map.  The maps are bit-equal to the reference's.  ``as_tensor`` (device path
    only): the results stay on the device as torch tensors instead of coming back as numpy arrays."""
    from . import _lib
    if as_tensor and device is None:
        raise ValueError("as_tensor needs a device")
    parts = np.ascontiguousarray(parts, dtype=np.float64)
    if parts.ndim != 3 or parts.shape[2] != 2:
        raise ValueError("parts must be [B, Kp, 2]")
    B, Kp = parts.shape[:2]
    ul = np.ascontiguousarray(ul, dtype=np.float32).reshape(-1, 2)
    br = np.ascontiguousarray(br, dtype=np.float32).reshape(-1, 2)
    if len(ul) != B or len(br) != B:
        raise ValueError("ul and br need one row per sample")
    inpH, inpW, resH, resW = int(in_res[0]), int(in_res[1]), int(out_res[0]), int(out_res[1])
    if min(inpH, inpW, resH, resW) < 1 or Kp < 1:
        raise ValueError("resolutions and Kp must be positive")
    if B * Kp * resH * ((resW + 3) // 4 * 4) >= 1 << 31:
        raise ValueError("the target tensor must hold fewer than 2^31 values")
    g = gaussian_table(sigma)
    if not B:
        out, centres = np.empty((B, Kp, resH, resW), np.float32), np.empty((B, Kp, 2), np.int32)
        return (out, centres, np.empty((B, Kp, resH, resW), np.float32)) if want_mask else (out, centres)
    side = _lib.Side(device)
    out, centres = side.empty((B, Kp, resH, resW), np.float32), side.empty((B, Kp, 2), np.int32)
    mask = side.empty((B, Kp, resH, resW), np.float32) if want_mask else None
    side.call("bp_kpd_targets", side.put(parts), side.put(ul), side.put(br), B, Kp, inpH, inpW, resH, resW, side.put(g), len(g),
              out, centres, mask)
    if not as_tensor:
        out, centres, mask = side.get(out), side.get(centres), side.get(mask) if want_mask else None
    return (out, centres, mask) if want_mask else (out, centres)


def kpd_windows(bndbox, scale_rate, image_size):
    """generateSampleBox's window (pose.py:30-41) of ``B`` boxes ``bndbox`` [B, 4] (x1, y1, x2, y2): the corners are
    truncated to integers, then widened by ``scale_rate / 2`` of the box's width and height on each side and clamped
    to the image ``image_size = (H, W)``, all in float32 as the reference's tensors are.  ``scale_rate`` (a number or
    [B]) is the caller's own draw of ``random.uniform(*scale_factor)``.  ``(ul [B, 2], br [B, 2])`` float32."""
    b = np.asarray(bndbox, dtype=np.float64).reshape(-1, 4)
    rate = np.broadcast_to(np.asarray(scale_rate, dtype=np.float64), (len(b),)).astype(np.float32)
    imght, imgwidth = np.float32(image_size[0]), np.float32(image_size[1])
    ul = np.trunc(b[:, 0:2]).astype(np.float32)
    br = np.trunc(b[:, 2:4]).astype(np.float32)
    ht, width = br[:, 1] - ul[:, 1], br[:, 0] - ul[:, 0]
    two, one, zero = np.float32(2), np.float32(1), np.float32(0)
    out_ul = np.stack([np.maximum(zero, ul[:, 0] - width * rate / two), np.maximum(zero, ul[:, 1] - ht * rate / two)], axis=1)
    out_br = np.stack([np.minimum(imgwidth - one, br[:, 0] + width * rate / two),
                       np.minimum(imght - one, br[:, 1] + ht * rate / two)], axis=1)
    return np.ascontiguousarray(out_ul, np.float32), np.ascontiguousarray(out_br, np.float32)


def reference_labels(xy, vertex_box, gt_box_xyxy):
    """The reference's saved ``kp_label`` from the true projections ``xy`` [P, Kp, 2]: project_kp stores each point as
    a ratio within ``mask_bbox`` (``vertex_box`` [P, 4], (xmin, xmax, ymin, ymax)), and ``output`` undoes the ratio
    against the GROUND-TRUTH box (``gt_box_xyxy`` [P, 4]) -- so the reference's label is the true projection rescaled
    from one box to the other.  Same operations in the same order, float64."""
    xy = np.asarray(xy, dtype=np.float64)
    vb = np.asarray(vertex_box, dtype=np.float64).reshape(-1, 1, 4)
    gb = np.asarray(gt_box_xyxy, dtype=np.float64).reshape(-1, 1, 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        xr = (xy[..., 0] - vb[..., 0]) / (vb[..., 1] - vb[..., 0])
        yr = (xy[..., 1] - vb[..., 2]) / (vb[..., 3] - vb[..., 2])
    return np.stack([xr * (gb[..., 2] - gb[..., 0]) + gb[..., 0], yr * (gb[..., 3] - gb[..., 1]) + gb[..., 1]], axis=-1)


def annotate_sequence(bench, obj_id, kp3d, faces=None, use_depth=False, reference=False, device=None, size=(480, 640)):
    """Annotate every frame of ``bench`` (sixd.load_sixd) that holds object ``obj_id``: a dict of arrays with one row per
    annotated frame, ``frames`` [N] (frame numbers), ``kp_label`` [N, Kp, 2], ``kp_depth`` [N, Kp], ``kp_flags``
    [N, Kp] (project_keypoints' bits) and ``bbox`` [N, 4] (ground truth, x1 y1 x2 y2, as the reference writes it).
    With ``faces`` (triangles of ``bench.models['%02d' % obj_id].vertices``) the mesh is rendered at every pose, self
    occlusion is marked and ``box_full``, ``box_visible`` [N, 4] (xmin, xmax, ymin, ymax) and ``visib_fract`` [N] are
    added; ``use_depth`` also tests against each frame's depth image (``load_sixd(load_depth=True)``).  ``reference``:
    ``kp_label`` is the reference's own (reference_labels through vertex_boxes) instead of the true projection."""
    name = "%02d" % int(obj_id)
    kp3d = np.ascontiguousarray(kp3d, dtype=np.float64).reshape(-1, 3)
    H, W = _size(size)
    nrs, poses, boxes, depth_of = [], [], [], []
    for fr in bench.frames:
        for oid, pose, bb in fr.gt:
            if int(oid) != int(obj_id):
                continue
            nrs.append(int(fr.nr))
            poses.append(np.asarray(pose, dtype=np.float64)[:3, :4])
            boxes.append([bb[0], bb[1], bb[0] + bb[2], bb[1] + bb[3]])
            depth_of.append(fr.depth)
    N = len(nrs)
    poses = np.asarray(poses, dtype=np.float64).reshape(N, 3, 4)
    ann = {"frames": np.asarray(nrs, dtype=np.int64), "bbox": np.asarray(boxes, dtype=np.float64).reshape(N, 4)}
    vertices = None
    if faces is not None or reference:
        if name not in bench.models:
            raise ValueError("bench.models has no mesh of object %s" % name)
        vertices = np.ascontiguousarray(bench.models[name].vertices, dtype=np.float64)
    if use_depth and any(d is None for d in depth_of):
        raise ValueError("use_depth needs the frames' depth images: load_sixd(..., load_depth=True)")
    K = bench.cam
    xy, z, flags = np.empty((N, len(kp3d), 2)), np.empty((N, len(kp3d))), np.empty((N, len(kp3d)), np.uint8)
    if faces is not None:
        ann.update(box_full=np.empty((N, 4), np.int32), box_visible=np.empty((N, 4), np.int32), visib_fract=np.zeros(N))
    step = max(1, (1 << 24) // (H * W))                    # frames per chunk, as pose_errors_vsd's host path
    for s in range(0, N, step):
        e = min(N, s + step)
        md = render_depth(poses[s:e], vertices, faces, K, (H, W), device)[0] if faces is not None else None
        scene = None
        if use_depth:
            scene = scene_depth_from_u16(np.stack([depth_of[i] for i in range(s, e)]), bench.scale_to_meters)
        xy[s:e], z[s:e], flags[s:e] = project_keypoints(poses[s:e], kp3d, K, (H, W), md, scene, device=device)
        if faces is not None:
            b, c = mask_boxes(md, K, scene, device=device)
            ann["box_full"][s:e], ann["box_visible"][s:e] = b[:, 0], b[:, 1]
            ann["visib_fract"][s:e] = c[:, 1] / np.maximum(c[:, 0], 1)
    ann["kp_label"] = reference_labels(xy, vertex_boxes(poses, vertices, K, (H, W), device), ann["bbox"]) if reference and N \
        else xy
    ann["kp_depth"], ann["kp_flags"] = z, flags
    return ann


def darknet_label(bbox_xyxy, image_size=(480, 640)):
    """One label line of train_YOLO/scripts/gt_single_object.py (class 0, box centre and size as fractions of the
    image) for a ground-truth box (x1, y1, x2, y2)."""
    x1, y1, x2, y2 = (float(v) for v in bbox_xyxy)
    w, h = x2 - x1, y2 - y1
    return "0 %f %f %f %f" % ((x1 + w / 2) / image_size[1], (y1 + h / 2) / image_size[0], w / image_size[1], h / image_size[0])


def darknet_labels_multi(gt_rows, class_of, image_size=(480, 640), box="full"):
    """The label lines of train_YOLO/scripts/gt_multi_object.py for one frame's ``gt.yml`` rows: one ``"%d %f %f %f %f"``
    line (class, box centre and size as fractions of the image) per row whose ``obj_id`` is a key of ``class_of``
    ({obj_id: class}), in row order.  ``box="full"`` reads ``obj_bb`` (x, y, w, h) -- with ``class_of = {i: i - 1}`` these
    are the reference's lines --, ``box="visible"`` reads ``obj_bb_visib`` (synth.write_scene_tree's) and raises where a
    row has none."""
    if box not in ("full", "visible"):
        raise ValueError("box must be 'full' or 'visible'")
    key = "obj_bb" if box == "full" else "obj_bb_visib"
    height, width = image_size
    lines = []
    for row in gt_rows:
        oid = int(row["obj_id"])
        if oid not in class_of:
            continue
        if key not in row:
            raise ValueError("a gt.yml row of object %d has no %s" % (oid, key))
        bbox = list(row[key])
        bbox[0] = (bbox[0] + bbox[2] / 2) / width
        bbox[1] = (bbox[1] + bbox[3] / 2) / height
        bbox[2] = bbox[2] / width
        bbox[3] = bbox[3] / height
        lines.append("%d %f %f %f %f" % (int(class_of[oid]), bbox[0], bbox[1], bbox[2], bbox[3]))
    return lines


def write_multi_labels(bench_or_tree, seq, outdir, class_of, train_split, seed=0, box="full", image_size=None):
    """Detector labels of EVERY object of a sequence: ``outdir/labels/NNNN.txt`` with darknet_labels_multi's lines for
    each frame (an empty file where none of ``class_of``'s objects is in the frame), a seeded random split of
    ``train_split`` frames for training and the rest for evaluation as ``train.txt`` / ``eval.txt`` (frame file names,
    as write_annotations), ``obj.names`` (``obj_XX`` per class, in class order) and ``obj.data`` with ``classes``,
    ``train``, ``valid``, ``names`` and ``backup``, the keys train_detector.py and detector_map.py read.
    ``bench_or_tree``: a SIXD tree's path, whose ``test/SS/gt.yml`` is read row by row (what ``box="visible"`` needs), or
    a sixd.load_sixd benchmark (full boxes only; ``seq`` is then unused).  ``image_size`` defaults to the tree's
    ``camera.yml`` (480 x 640 without one).  Returns ``{'train': [...], 'eval': [...]}``, the frame numbers."""
    import yaml
    class_of = {int(k): int(v) for k, v in class_of.items()}
    classes = sorted(set(class_of.values()))
    if classes != list(range(len(classes))) or len(classes) != len(class_of):
        raise ValueError("class_of must map the objects one to one onto classes 0 .. n - 1")
    if isinstance(bench_or_tree, (str, os.PathLike)):
        tree = os.fspath(bench_or_tree)
        with open(os.path.join(tree, "test", "%02d" % int(seq), "gt.yml")) as f:
            rows_of = {int(nr): rows for nr, rows in yaml.safe_load(f).items()}
        if image_size is None and os.path.exists(os.path.join(tree, "camera.yml")):
            with open(os.path.join(tree, "camera.yml")) as f:
                cam = yaml.safe_load(f)
            image_size = (int(cam.get("height", 480)), int(cam.get("width", 640)))
    else:
        rows_of = {int(fr.nr): [{"obj_id": int(o), "obj_bb": list(bb)} for o, _, bb in fr.gt] for fr in bench_or_tree.frames}
    image_size = (480, 640) if image_size is None else image_size
    frames = sorted(rows_of)
    N = len(frames)
    if not 0 <= int(train_split) <= N:
        raise ValueError("train_split must lie in 0 .. %d" % N)
    os.makedirs(os.path.join(outdir, "labels"), exist_ok=True)
    for nr in frames:
        with open(os.path.join(outdir, "labels", "%04d.txt" % nr), "w") as f:
            f.write("".join(ln + "\n" for ln in darknet_labels_multi(rows_of[nr], class_of, image_size, box)))
    chosen = set(np.random.default_rng(seed).choice(N, int(train_split), replace=False).tolist()) if N else set()
    split = {"train": [nr for i, nr in enumerate(frames) if i in chosen], "eval": [nr for i, nr in enumerate(frames) if i not in chosen]}
    for t, nrs in split.items():
        with open(os.path.join(outdir, "%s.txt" % t), "w") as f:
            f.write("".join("%04d.png\n" % nr for nr in nrs))
    write_detector_data(outdir, class_of)
    return split


def write_detector_data(folder, class_of):
    """``obj.names`` and ``obj.data`` of the detector set in ``folder`` (its ``train.txt`` / ``eval.txt``)."""
    by_class = sorted((c, o) for o, c in class_of.items())
    with open(os.path.join(folder, "obj.names"), "w") as f:
        f.write("".join("obj_%02d\n" % o for _, o in by_class))
    with open(os.path.join(folder, "obj.data"), "w") as f:
        f.write("classes = %d\ntrain = %s\nvalid = %s\nnames = %s\nbackup = %s\n" % (
            len(by_class), os.path.join(folder, "train.txt"), os.path.join(folder, "eval.txt"), os.path.join(folder, "obj.names"),
            os.path.join(folder, "backup")))


def write_annotations(outdir, ann, train_split, seed=0, image_size=(480, 640)):
    """Write ``ann`` (annotate_sequence) in the reference's layout under ``outdir``: ``kp_label/<i>.npy`` [Kp, 2] and
    ``bbox/<i>.npy`` [4] per annotated frame (``i`` counts the annotations from 0, the reference's output_counter), a
    seeded random split of ``train_split`` frames for training and the rest for evaluation, ``annot_train.npz`` and
    ``annot_eval.npz`` with the reference's three data sets -- ``bndbox`` [N, 1, 4], ``imgname`` [N, L] (character
    codes of ``'%012d.png' % frame``) and ``part`` [N, Kp, 2] -- plus ``flags`` [N, Kp], the same three as
    ``annot_*.h5`` when h5py is installed, and ``labels/<frame %04d>.txt`` with one Darknet line per frame
    (darknet_label).  Returns ``{'train': [...], 'eval': [...]}``, the annotation indices of the two sets."""
    N = len(ann["frames"])
    if not 0 <= int(train_split) <= N:
        raise ValueError("train_split must lie in 0 .. %d" % N)
    for sub in ("kp_label", "bbox", "labels"):
        os.makedirs(os.path.join(outdir, sub), exist_ok=True)
    for i in range(N):
        np.save(os.path.join(outdir, "kp_label", "%d.npy" % i), ann["kp_label"][i])
        np.save(os.path.join(outdir, "bbox", "%d.npy" % i), ann["bbox"][i])
        with open(os.path.join(outdir, "labels", "%04d.txt" % int(ann["frames"][i])), "w") as f:
            f.write(darknet_label(ann["bbox"][i], image_size) + "\n")
    chosen = set(np.random.default_rng(seed).choice(N, int(train_split), replace=False).tolist()) if N else set()
    split = {"train": [i for i in range(N) if i in chosen], "eval": [i for i in range(N) if i not in chosen]}
    Kp = ann["kp_label"].shape[1]
    for t, ids in split.items():
        names = ["%012d.png" % int(ann["frames"][i]) for i in ids]
        data = {"bndbox": ann["bbox"][ids].reshape(-1, 1, 4),
                "imgname": np.array([[ord(c) for c in n] for n in names], dtype=np.int64).reshape(len(ids), 16),
                "part": ann["kp_label"][ids].reshape(-1, Kp, 2)}
        np.savez(os.path.join(outdir, "annot_%s.npz" % t), flags=ann["kp_flags"][ids], **data)
        with open(os.path.join(outdir, "%s.txt" % t), "w") as f:
            f.write("".join(n + "\n" for n in names))
        try:
            import h5py
        except ImportError:
            continue
        with h5py.File(os.path.join(outdir, "annot_%s.h5" % t), "w") as f:
            for k, v in data.items():
                f.create_dataset(k, data=v)
    return split
