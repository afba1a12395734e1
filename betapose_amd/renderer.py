"""Posed meshes in colour: the call surface of the reference's ``utils/renderer.py`` (``Renderer.draw_model``,
``draw_boundingbox``, ``finish``) and of ``utils/utils.py:269 draw_detections_3D`` over metrics.render_color, draw_boxes and
overlay (csrc/raster_color.hip on a device, its host twin without one; the two are byte-identical).  There is no OpenGL
here: DESIGN.md 3.5 defines the image and lists where it departs from the reference's.

A ``model`` is any object with ``vertices`` [n, 3], ``indices`` [F, 3], ``colors`` [n, 3] floats in [0, 1] (in the channel
order the caller wants back) and ``bb`` [8, 3] (``metrics.Model3D.load_mesh`` fills them); ``bb_colors`` [8, 3] floats is
optional (default: the reference's corner colours as RGB)."""
from __future__ import annotations

import numpy as np

from . import metrics


def _pose34(pose):
    return np.asarray(pose, dtype=np.float64)[:3, :4]


def _box_colors(model, flip=False):
    c = np.asarray(getattr(model, "bb_colors", metrics.BOX_CORNER_COLORS), dtype=np.float64).reshape(8, 3)
    return metrics.colors_u8(c[:, ::-1] if flip else c)


class Renderer:
    """``Renderer(size, cam, device=None)``, ``size = (width, height)`` as in the reference.  ``draw_model`` calls
    accumulate behind one z-buffer, ``draw_boundingbox`` calls are applied on top at ``finish``, which returns
    ``(rgb float32 [H, W, 3] in [0, 1], depth float32 [H, W])``: background colour 0, depth 0.  The depth is the meshes';
    box lines carry none (``drawn`` [H, W] bool marks every pixel a mesh or a box touched).  Pixel centres lie at
    (x + 0.5, y + 0.5), the reference renderer's convention.  ``clip_far`` is accepted and unused: no far plane."""

    pixel_center = 0.5

    def __init__(self, size, cam, device=None):
        self.size = (int(size[0]), int(size[1]))
        self.shape = (self.size[1], self.size[0])
        self.device = device
        self.set_cam(cam)
        self.clear()

    def set_cam(self, cam, clip_near=0.01, clip_far=10.0):
        self.cam = np.asarray(cam, dtype=np.float64).reshape(3, 3)
        self.clip_near = float(clip_near)
        self.clip_far = float(clip_far)

    def clear(self):
        self._color = np.zeros((1,) + self.shape + (3,), np.uint8)
        self._depth = np.zeros((1,) + self.shape, np.float32)
        self._boxes = []
        self.drawn = np.zeros(self.shape, bool)

    def draw_model(self, model, pose, ambient_weight=0.5, light=(0, 0, 0)):
        self._color, self._depth, _ = metrics.render_color(
            _pose34(pose)[None], model.vertices, model.indices, metrics.colors_u8(model.colors), self.cam, self.shape,
            self.device, image_index=[0], images=1, pixel_center=self.pixel_center, near=self.clip_near,
            ambient=ambient_weight, light=light, into=(self._color, self._depth))

    def draw_boundingbox(self, model, pose):
        self._boxes.append((np.asarray(model.bb, dtype=np.float64).reshape(8, 3), _box_colors(model), _pose34(pose)))

    def finish(self):
        color, touched = draw_box_lines(self._color, self._boxes, self.cam, self.device, self.pixel_center, self.clip_near)
        self.drawn = (self._depth[0] > 0) | touched[0]
        return color[0].astype(np.float32) / np.float32(255.0), self._depth[0].copy()


WHITE = np.full((8, 3), 255, np.uint8)


def draw_box_lines(color, boxes, cam, device=None, pixel_center=0.5, near=0.01):
    """``boxes``: (corners [8, 3], corner colours [8, 3] uint8, pose [3, 4]) triples, all for image 0 of ``color``
    [1, H, W, 3] uint8.  Returns (the image with the lines on top, later boxes over earlier ones, and the mask
    [1, H, W] of the pixels a line touched).  The mask is one more draw_boxes call per run of boxes that share corners:
    white lines over a black image."""
    touched = np.zeros(color.shape[:3], bool)
    k = 0
    while k < len(boxes):
        corners, cc = boxes[k][0], boxes[k][1]
        run = [boxes[k][2]]
        k += 1
        while k < len(boxes) and np.array_equal(boxes[k][0], corners) and np.array_equal(boxes[k][1], cc):
            run.append(boxes[k][2])
            k += 1
        poses, index = np.stack(run), np.zeros(len(run), np.int32)
        color = metrics.draw_boxes(color, poses, corners, cam, cc, device, index, pixel_center, near)
        touched |= metrics.draw_boxes(np.zeros_like(color), poses, corners, cam, WHITE, device, index, pixel_center, near).any(axis=-1)
    return color, touched


def draw_detections_3D(image, detections, cam, model_map, thres):
    """Signature and behaviour of the reference's function of this name: ``detections`` is a score-ordered list of
    ``[class index, confidence, l, t, r, b, pose0, ..., poseN]``; the 3-D box of every pose of every detection ahead of
    the first one scoring under ``thres`` is drawn with the model ``model_map["%02d" % (class index + 1)]``, and the lines
    replace the pixels of a copy of ``image`` (floats in [0, 1]); everything else is ``image``.  Pixel centres at +0.5."""
    result = np.array(image, copy=True)
    scores = [d[1] for d in detections]
    shown = next((i for i, sc in enumerate(scores) if sc < thres), len(scores))
    boxes = []
    for det in detections[:shown]:
        model = model_map["%02d" % (int(det[0]) + 1)]
        boxes += [(np.asarray(model.bb, dtype=np.float64).reshape(8, 3), _box_colors(model), _pose34(T)) for T in det[6:]]
    if boxes:
        blank = np.zeros((1,) + tuple(image.shape[:2]) + (3,), np.uint8)
        lines, touched = draw_box_lines(blank, boxes, cam, pixel_center=Renderer.pixel_center)
        result[touched[0]] = lines[0][touched[0]].astype(result.dtype) / 255.0
    return result


def draw_scene(frames_u8, groups, cam, alpha=128, device=None, pixel_center=0.0, near=0.01):
    """Frames [I, H, W, 3] uint8 with posed models drawn over them, in one batch of calls.  ``groups``: dicts with
    ``model``, ``poses`` [P, 3|4, 4], ``image_index`` [P] (non-decreasing) and optionally ``mesh`` (default True: the
    shaded mesh is blended at ``alpha``), ``box`` (default True), ``box_colors`` [8, 3] uint8 and ``flip`` (True: the
    model's RGB colours are written as BGR).  All meshes share one z-buffer per frame; the boxes go on top, in the order of
    the groups."""
    frames = np.ascontiguousarray(frames_u8, dtype=np.uint8)
    I, H, W = frames.shape[:3]
    state = None
    for g in groups:
        if not g.get("mesh", True) or len(g["poses"]) == 0:
            continue
        m = g["model"]
        col = np.asarray(m.colors, dtype=np.float64)
        col = metrics.colors_u8(col[:, ::-1] if g.get("flip") else col)
        color, depth, _ = metrics.render_color(g["poses"], m.vertices, m.indices, col, cam, (H, W), device,
                                               image_index=g["image_index"], images=I, pixel_center=pixel_center,
                                               near=near, into=state)
        state = (color, depth)
    out = frames if state is None else metrics.overlay(frames, state[0], state[1], alpha, device)
    for g in groups:
        if not g.get("box", True) or len(g["poses"]) == 0:
            continue
        cc = g.get("box_colors")
        if cc is None:
            cc = _box_colors(g["model"], g.get("flip", False))
        out = metrics.draw_boxes(out, g["poses"], g["model"].bb, cam, cc, device, g["image_index"], pixel_center, near)
    return out


def draw_poses(image_bgr_u8, poses, model, cam, alpha=128, box=True, device=None):
    """``image_bgr_u8`` [H, W, 3] with ``model`` (RGB colours) at every pose of ``poses`` blended over it at ``alpha``
    (0 .. 256) and, with ``box``, its 3-D boxes on top: what the harness writes for ``--save_img``."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, *np.shape(poses)[-2:])
    g = {"model": model, "poses": poses, "image_index": np.zeros(len(poses), np.int32), "box": box, "flip": True}
    return draw_scene(np.asarray(image_bgr_u8)[None], [g], cam, alpha, device)[0]


GREEN = np.tile(np.array([[0, 255, 0]], np.uint8), (8, 1))       # the ground-truth box (RGB and BGR alike)


def _pose44(R, t):
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
    return pose


def frame_poses(frame, all_instances=False):
    """The solved poses [4, 4] of one frame dict of ``final_result``: its ``cam_R`` / ``cam_t`` (the refined pose after
    --refine_depth), or with ``all_instances`` those of every solved entry of its ``"instances"``."""
    if all_instances and "instances" in frame:
        return [_pose44(s["cam_R"], s["cam_t"]) for s in frame["instances"] if int(s["status"]) == 0 and len(s["cam_R"]) > 0]
    if len(frame["result"]) < 1 or len(frame["cam_R"]) == 0:
        return []
    return [_pose44(frame["cam_R"], frame["cam_t"])]


def _image_u8(image):
    """A frame as uint8 [H, W, 3]: uint8 as it is, floats in [0, 1] rounded to nearest."""
    image = np.asarray(image)
    return np.ascontiguousarray(image if image.dtype == np.uint8 else metrics.colors_u8(image))


def verify_6D_poses(detections, model_map, cam, image, device=None):
    """Signature and behaviour of the reference's function of this name (utils/utils.py:558-610): ``detections`` is a
    list of ``[class index, confidence, l, t, r, b, pose0, ..., poseN]`` for one ``image`` ([H, W, 3], BGR as the
    reference reads frames: uint8, or floats in [0, 1]); every pose of a detection is rendered with the model
    ``model_map["%02d" % (class index + 1)]`` and scored by the agreement of its unit Sobel gradients with the image's
    (metrics.verify_poses with the reference's thresholds and this module's ``Renderer`` pixel centre, ambient weight
    and light); returned is the list of ``det[:6] + [best pose]``, the first pose on a tie as ``np.argmax``.  The gray
    conversion treats byte 2 as red for the image and for the render, as the reference's ``COLOR_BGR2GRAY`` does to both.
    ``device``: None for the host twin, a torch device for the GPU; the choice is the same.  DESIGN.md 3.18 lists where
    the score departs from the reference's."""
    frame = _image_u8(image)[None]
    filtered = []
    for det in detections:
        model = model_map["%02d" % (int(det[0]) + 1)]
        poses = [_pose34(T) for T in det[6:]]
        new_det = list(det[:6])
        if poses:
            scores = metrics.verify_poses(np.stack(poses), model.vertices, model.indices, metrics.colors_u8(model.colors),
                                          cam, frame, np.zeros(len(poses), np.int32), device,
                                          pixel_center=Renderer.pixel_center, red_channel=2)[0]
            new_det.append(det[6 + int(np.argmax(scores))])
        filtered.append(new_det)
    return filtered


def verify_results(final_result, model, frame_dir, cam, device=None, batch=8):
    """--verify: for every frame dict of ``final_result`` whose ``"instances"`` list has at least two solved entries,
    those poses are rendered with ``model`` (RGB colours) and scored against the frame ``<frame_dir>/<imgname>``
    (metrics.verify_poses, pixel centre 0).  Every solved instance gets its score as ``"verify_score"``; the pose with
    the highest score (the first on a tie) becomes the frame's ``cam_R`` / ``cam_t`` and the pose it replaces is kept
    under ``"pose_unverified"`` = ``{"cam_R", "cam_t"}``.  Frames with fewer solved instances are left untouched.
    Frames are read and scored ``batch`` at a time on ``device`` (None: the host twin; same choice, same bytes).
    Returns ``(frames scored, choices changed)``."""
    import os
    from PIL import Image
    todo = []
    for f in final_result:
        solved = [k for k, s in enumerate(f.get("instances", ())) if int(s["status"]) == 0 and len(s["cam_R"]) > 0]
        if len(solved) >= 2:
            todo.append((f, solved))
    changed = 0
    colors = metrics.colors_u8(model.colors)
    for b0 in range(0, len(todo), batch):
        part = todo[b0:b0 + batch]
        frames = [np.asarray(Image.open(os.path.join(frame_dir, os.path.basename(f["imgname"]))).convert("RGB")) for f, _ in part]
        groups = [list(range(len(part)))] if len({fr.shape for fr in frames}) == 1 else [[i] for i in range(len(part))]
        for slots in groups:
            poses, index = [], []
            for k, i in enumerate(slots):
                f, solved = part[i]
                for j in solved:
                    poses.append(_pose44(f["instances"][j]["cam_R"], f["instances"][j]["cam_t"]))
                    index.append(k)
            scores = metrics.verify_poses(np.stack(poses), model.vertices, model.indices, colors, cam,
                                          np.stack([frames[i] for i in slots]), np.array(index, np.int32), device)[0]
            at = 0
            for i in slots:
                f, solved = part[i]
                sc = scores[at:at + len(solved)]
                at += len(solved)
                for j, v in zip(solved, sc):
                    f["instances"][j]["verify_score"] = float(v)
                best = f["instances"][solved[int(np.argmax(sc))]]
                old_R, old_t = np.asarray(f["cam_R"], dtype=np.float64), np.asarray(f["cam_t"], dtype=np.float64)
                new_R = np.asarray(best["cam_R"], dtype=np.float64).reshape(old_R.shape if old_R.size == 9 else (3, 3))
                new_t = np.asarray(best["cam_t"], dtype=np.float64).reshape(old_t.shape if old_t.size == 3 else (3, 1))
                f["pose_unverified"] = {"cam_R": f["cam_R"], "cam_t": f["cam_t"]}
                if old_R.size != 9 or not (np.array_equal(new_R, old_R) and np.array_equal(new_t, old_t)):
                    changed += 1
                f["cam_R"], f["cam_t"] = new_R, new_t
    return len(todo), changed


class BoxModel:
    """A grey box around ``points`` as a renderer model: what --save_img draws where there is no mesh file (--synthetic)."""

    def __init__(self, points):
        self.bb = metrics.box_corners(points)
        self.vertices = self.bb
        self.indices = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6],
                                 [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
        self.colors = np.full((8, 3), 0.5)


def save_pose_images(objects, frame_dir, out_dir, cam, device=None, all_instances=False, batch=8, alpha=128):
    """--save_img: ``<out_dir>/vis/<imgname>.png`` for every frame in which any object has a solved pose: the frame with
    every such pose's mesh blended over it at ``alpha``, its 3-D box and, where ground truth is given, the ground-truth
    box in green.  ``objects``: dicts with ``model``, ``results`` (a ``final_result`` list) and optionally ``gt``
    (frame number -> [{"pose"}]).  Frames are rendered ``batch`` at a time, one render_color call per object and batch
    (``image_index``), on ``device`` (None: the host twin).  Returns the number of images written."""
    import os
    from PIL import Image
    per_frame = {}
    for oi, obj in enumerate(objects):
        for f in obj["results"]:
            poses = frame_poses(f, all_instances)
            if poses:
                per_frame.setdefault(os.path.basename(f["imgname"]), {})[oi] = poses
    names = sorted(per_frame)
    vis = os.path.join(out_dir, "vis")
    if names:
        os.makedirs(vis, exist_ok=True)
    for b0 in range(0, len(names), batch):
        chunk = names[b0:b0 + batch]
        frames = [np.asarray(Image.open(os.path.join(frame_dir, n)).convert("RGB")) for n in chunk]
        if len({fr.shape for fr in frames}) > 1:            # frames of one size per call: fall back to one at a time
            groups_of = [[i] for i in range(len(chunk))]
        else:
            groups_of = [list(range(len(chunk)))]
        for slots in groups_of:
            groups = []
            for oi, obj in enumerate(objects):
                est, est_i, gts, gts_i = [], [], [], []
                for k, i in enumerate(slots):
                    for pose in per_frame[chunk[i]].get(oi, []):
                        est.append(pose)
                        est_i.append(k)
                    nr = os.path.splitext(chunk[i])[0]
                    if obj.get("gt") is not None and nr.isdigit() and oi in per_frame[chunk[i]]:
                        for g in obj["gt"].get(int(nr), []):
                            gts.append(g["pose"])
                            gts_i.append(k)
                if est:
                    groups.append({"model": obj["model"], "poses": np.array(est), "image_index": np.array(est_i, np.int32)})
                if gts:
                    groups.append({"model": obj["model"], "poses": np.array(gts), "image_index": np.array(gts_i, np.int32),
                                   "mesh": False, "box_colors": GREEN})
            out = draw_scene(np.stack([frames[i] for i in slots]), groups, cam, alpha, device)
            for k, i in enumerate(slots):
                Image.fromarray(out[k]).save(os.path.join(vis, os.path.splitext(chunk[i])[0] + ".png"), format="PNG")
    return len(names)
