#!/usr/bin/env python3
"""Generate tests/golden/annot.npz by running the REFERENCE's own Python (build container only, like tools/make_golden.py;
nothing of the reference is copied, it is imported in place under stubs for the packages that are not installed).

  annotator  ``2_keypoint_annotator/annotate_keypoint.py`` is imported whole (its ``__main__`` block does not run): the
             ``sinobj`` methods apply_pose, project_all, project_kp and output are driven on a few hundred random
             vertices, 9 key points and 6 poses with LineMod's camera at 480 x 640 -> ``mask_bbox``, the ``kp_2d``
             ratios and the saved ``kp_label`` / ``bbox`` files.
  targets    ``train_KPD/src/utils/img.py`` transformBox and drawGaussian on 40 (window, part) cases at 320 x 256 ->
             80 x 64 with hmGauss = 1.  generateSampleBox itself loads an image and draws random numbers, so only its
             test ``part.x > 0 and ul < part < br`` is restated around the two functions (said in ``meta``).

Conditions the generator enforces by redrawing, so that the tests need no carve-out: no projected vertex within 1e-6 px
of an integer, no part within 1e-3 px of a window edge, no pre-round heat-map coordinate (recomputed in float64) within
1e-3 of a half-integer.

The archive is written with fixed time stamps: running this twice gives the same bytes.

Usage: python tools/make_golden_annot.py
"""
from __future__ import annotations

import importlib.util
import io
import json
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_shims  # noqa: E402  (only for where the reference lies; its install() is not used here)

REF = os.path.dirname(ref_shims.REF)
ANNOTATOR = os.path.join(REF, "2_keypoint_annotator")
KPD_IMG = os.path.join(REF, "3_6Dpose_estimator", "train_KPD", "src", "utils", "img.py")
K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
H, W = 480, 640
SEED = 20
stubbed = []


class _Permissive(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: 0


def _stub(name, **attrs):
    m = _Permissive(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    stubbed.append(name)
    return m


def import_annotator():
    """annotate_keypoint.py as a module.  Its utils/ files import each other by bare name (Python 2 style), so that
    directory goes on the path behind the annotator's own, and the one name the package itself is asked for
    (``from utils import output_pointcloud``, utils/model.py) is set on the package beforehand."""
    sys.dont_write_bytecode = True
    sys.argv = ["annotate_keypoint.py"]
    sys.path.insert(0, os.path.join(ANNOTATOR, "utils"))
    sys.path.insert(0, ANNOTATOR)
    for name in ("cv2", "h5py", "IPython", "OpenGL", "OpenGL.GL"):
        _stub(name)
    _stub("plyfile", PlyData=object)
    vis = _stub("vispy")
    vis.app = _stub("vispy.app", Canvas=object)
    vis.gloo = _stub("vispy.gloo")
    import utils as ref_utils_pkg
    import utils.utils as ref_utils
    ref_utils_pkg.output_pointcloud = ref_utils.output_pointcloud
    import annotate_keypoint
    return annotate_keypoint, ref_utils


def import_kpd_img():
    """train_KPD's utils/img.py under a name of its own (``utils`` and ``opt`` mean the annotator's by now)."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "opt" or k == "utils" or k.startswith("utils.")}
    _stub("opt", opt=types.SimpleNamespace())
    _stub("scipy.misc")
    ts = _stub("torchsample")
    ts.transforms = _stub("torchsample.transforms", SpecialCrop=object, Pad=object)
    spec = importlib.util.spec_from_file_location("ref_train_kpd_img", KPD_IMG)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    del sys.modules["opt"]
    sys.modules.update(saved)
    return mod


def rand_rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def project(pose, pts):
    X = pts @ pose[:3, :3].T + pose[:3, 3]
    return np.stack([X[:, 0] * K[0, 0] / X[:, 2] + K[0, 2], X[:, 1] * K[1, 1] / X[:, 2] + K[1, 2]], axis=1)


def draw_scene(rng):
    """vertices [300, 3], key points [9, 3] (metres) and 6 poses: four in view, one cut by the left image border, one by
    the bottom one; redrawn until no projected vertex lies within 1e-6 px of an integer."""
    while True:
        vertices = rng.uniform(-1, 1, (300, 3)) * np.array([0.06, 0.045, 0.03])
        kp3d = rng.uniform(-1, 1, (9, 3)) * np.array([0.05, 0.04, 0.025])
        poses = np.tile(np.eye(4), (6, 1, 1))
        for p in range(6):
            z = rng.uniform(0.5, 1.0)
            poses[p, :3, :3] = rand_rot(rng)
            poses[p, :3, 3] = [rng.uniform(-0.15, 0.15) * z, rng.uniform(-0.1, 0.1) * z, z]
        poses[4, :3, 3] = [-K[0, 2] / K[0, 0] * 0.6, 0.02, 0.6]              # centred on the left border
        poses[5, :3, 3] = [0.05, (H - K[1, 2]) / K[1, 1] * 0.7, 0.7]         # centred on the bottom border
        uv = np.concatenate([project(poses[p], vertices) for p in range(6)])
        if np.abs(uv - np.rint(uv)).min() > 1e-6:
            return vertices, kp3d, poses


def run_annotator(ak, vertices, kp3d, poses, gt_boxes):
    out = {"mask_bbox": [], "kp_2d": [], "kp_label": [], "bbox": []}
    with tempfile.TemporaryDirectory() as tmp:
        ak.output_kp_label_dir = os.path.join(tmp, "kp_label")
        ak.output_bbox_dir = os.path.join(tmp, "bbox")
        os.makedirs(ak.output_kp_label_dir)
        os.makedirs(ak.output_bbox_dir)
        ak.output_counter = 0
        for p in range(len(poses)):
            obj = ak.sinobj(1, list(gt_boxes[p]), poses[p])
            obj.apply_pose(vertices, kp3d)
            obj.project_all(K)
            obj.project_kp(K)
            obj.output(None)
            out["mask_bbox"].append([int(v) for v in obj.mask_bbox])
            out["kp_2d"].append(np.array(obj.kp_2d, dtype=np.float64))
            out["kp_label"].append(np.load(os.path.join(ak.output_kp_label_dir, "%d.npy" % p)))
            out["bbox"].append(np.load(os.path.join(ak.output_bbox_dir, "%d.npy" % p)))
    return {"mask_bbox": np.array(out["mask_bbox"], dtype=np.int32), "kp_2d": np.array(out["kp_2d"]),
            "kp_label": np.array(out["kp_label"], dtype=np.float64), "bbox": np.array(out["bbox"], dtype=np.float64)}


INP_H, INP_W, RES_H, RES_W = 320, 256, 80, 64


def heat_coords64(part, ul, br):
    """transformBox's coordinates before rounding, in float64."""
    ul, br = ul.astype(np.float64), br.astype(np.float64)
    centre = (br - 1 - ul) / 2
    lenH = max(br[1] - ul[1], (br[0] - ul[0]) * INP_H / INP_W)
    lenW = lenH * INP_W / INP_H
    pt = part - ul
    pt = pt + np.maximum(0, np.array([(lenW - 1) / 2 - centre[0], (lenH - 1) / 2 - centre[1]]))
    return pt * RES_H / lenH


def target_ok(part, ul, br):
    edges = np.abs(np.concatenate([part - ul.astype(np.float64), part - br.astype(np.float64)]))
    if edges.min() < 1e-3 or abs(part[0]) < 1e-3:
        return False
    q = heat_coords64(part, ul, br)
    return bool(np.abs(q - np.floor(q) - 0.5).min() > 1e-3)


def target_cases(rng):
    """40 (ul, br, part, what) cases; every fixed case is jittered by a fraction of a pixel until target_ok holds."""
    exact = (np.array([100, 50], np.float32), np.array([356, 370], np.float32))      # 256 x 320: window == map x 4
    wide = (np.array([100, 200], np.float32), np.array([400, 300], np.float32))      # the width arm of max(...)
    tall = (np.array([200, 50], np.float32), np.array([300, 400], np.float32))       # the height arm
    neg = (np.array([-10, 20], np.float32), np.array([200, 300], np.float32))        # a window that starts left of x = 0
    fixed = [
        (exact, (103, 200), "clipped left"), (exact, (353, 200), "clipped right"), (exact, (230, 53), "clipped top"),
        (exact, (230, 367), "clipped bottom"), (exact, (102, 52), "clipped corner top-left"),
        (exact, (354, 368), "clipped corner bottom-right"), (exact, (354, 52), "clipped corner top-right"),
        (exact, (228, 210), "interior"), (exact, (101.2, 300), "centre on column 0"),
        (wide, (250, 250), "wide interior"), (wide, (101.5, 201.5), "wide near corner"), (wide, (398, 298), "wide far corner"),
        (tall, (250, 225), "tall interior"), (tall, (201.5, 51.5), "tall near corner"), (tall, (298.5, 398.5), "tall far corner"),
        (exact, (90, 200), "outside left"), (exact, (370, 200), "outside right"), (exact, (230, 40), "outside above"),
        (exact, (230, 380), "outside below"), (wide, (50, 50), "outside both"),
        (neg, (-3, 100), "x <= 0 inside the window"), (neg, (0, 100), "x == 0"), (exact, (-20, 200), "x <= 0 outside"),
        (neg, (5, 100), "x > 0 in a window from x < 0"),
    ]
    cases = []
    for (ul, br), part, what in fixed:
        part = np.array(part, dtype=np.float64)
        exact_zero = what == "x == 0"
        while True:
            cand = part if exact_zero else part + rng.uniform(-0.2, 0.2, 2)
            if exact_zero or target_ok(cand, ul, br):
                cases.append((ul, br, cand, what))
                break
    while len(cases) < 40:
        ul = np.floor(rng.uniform(0, 300, 2)).astype(np.float32)
        br = (ul + np.floor(rng.uniform(40, 330, 2))).astype(np.float32)
        part = rng.uniform(ul - 15, br + 15)
        if target_ok(part, ul, br):
            cases.append((ul, br, part, "random"))
    return cases


def run_targets(img, cases):
    import torch
    out = {"t_ul": [], "t_br": [], "t_part": [], "t_drawn": [], "t_centre": [], "t_map": []}
    for ul, br, part, _ in cases:
        tul, tbr = torch.from_numpy(ul.copy()), torch.from_numpy(br.copy())
        # generateSampleBox's test, restated (train_KPD/src/utils/pose.py:116-117)
        drawn = bool(part[0] > 0 and part[0] > tul[0] and part[1] > tul[1] and part[0] < tbr[0] and part[1] < tbr[1])
        hm = torch.zeros(RES_H, RES_W)
        centre = np.array([-1, -1], dtype=np.int32)
        if drawn:
            hm_part = img.transformBox(part, tul, tbr, INP_H, INP_W, RES_H, RES_W)
            centre = hm_part.numpy().astype(np.int32)
            hm = img.drawGaussian(hm, hm_part, 1)
        out["t_ul"].append(ul)
        out["t_br"].append(br)
        out["t_part"].append(part)
        out["t_drawn"].append(drawn)
        out["t_centre"].append(centre)
        out["t_map"].append(hm.numpy().astype(np.float32))
    return {k: np.array(v) for k, v in out.items()}


def save_npz_fixed(path, arrays):
    """np.savez_compressed's format with every member stamped 1980-01-01, so the bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    rng = np.random.default_rng(SEED)
    vertices, kp3d, poses = draw_scene(rng)
    ak, _ = import_annotator()
    # ground-truth boxes as LineMod gives them (integers, x y w h -> x1 y1 x2 y2 as gene_all_files turns them), a few
    # pixels off the vertex box so that the box-to-box rescaling of the labels shows
    gt = []
    for p in range(6):
        uv = project(poses[p], vertices)
        x1, y1 = np.floor(uv.min(axis=0)) + rng.integers(-4, 5, 2)
        x2, y2 = np.ceil(uv.max(axis=0)) + rng.integers(-4, 5, 2)
        gt.append([float(x1), float(y1), float(x2), float(y2)])
    gt = np.array(gt)
    out = run_annotator(ak, vertices, kp3d, poses, gt)
    img = import_kpd_img()
    cases = target_cases(rng)
    out.update(run_targets(img, cases))
    import torch
    meta = {
        "generator": "tools/make_golden_annot.py", "seed": SEED, "numpy": np.__version__, "torch": torch.__version__,
        "reference_ran": ["2_keypoint_annotator/annotate_keypoint.py: sinobj.apply_pose, project_all, project_kp, output",
                          "2_keypoint_annotator/utils/utils.py: trans_vertices_by_pose, generate_mask_img, get_bbox_from_mask",
                          "3_6Dpose_estimator/train_KPD/src/utils/img.py: transformBox, drawGaussian"],
        "restated": ["train_KPD/src/utils/pose.py generateSampleBox: only its test `part.x > 0 and ul < part < br` around "
                     "transformBox / drawGaussian (the function loads an image and draws random numbers)",
                     "gene_all_files: the x y w h -> x1 y1 x2 y2 conversion of the ground-truth box"],
        "stubbed_third_party": sorted(set(stubbed)),
        "conditions": {"vertex_integer_margin_px": 1e-6, "part_window_margin_px": 1e-3, "half_integer_margin": 1e-3,
                       "exempt_cases": 0},
        "target_cases": [c[3] for c in cases],
        "resolution": [INP_H, INP_W, RES_H, RES_W], "hmGauss": 1,
    }
    out.update(vertices=vertices, kp3d=kp3d, poses=poses, K=K, size=np.array([H, W]), gt_bbox=gt,
               meta=np.array(json.dumps(meta, sort_keys=True)))
    path = os.path.join(ROOT, "tests", "golden", "annot.npz")
    save_npz_fixed(path, out)
    print(path, os.path.getsize(path), "bytes;", int(out["t_drawn"].sum()), "of", len(cases), "parts drawn")


if __name__ == "__main__":
    main()
