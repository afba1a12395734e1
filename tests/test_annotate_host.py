"""The host side of the key-point annotator (csrc/annotate_host.cpp through the bp_*_host entry points,
betapose_amd/annotate.py, annotate.py): the reference's own outputs from tests/golden/annot.npz (mask_bbox, kp_label,
bbox, transformBox centres and drawGaussian maps), visibility on constructed cases, the mask boxes against a numpy
restatement and against pose_errors_vsd's counts, the argument checks and the command-line tool.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import annotate_common as ac
import raster_common as rc
from betapose_amd import _lib, annotate as A, metrics, synth

ROOT = ac.ROOT
FRONT, IN_IMAGE, SELF, SCENE, KNOWN = ac.FRONT, ac.IN_IMAGE, ac.SELF, ac.SCENE, ac.KNOWN


def test_fixture_says_what_ran():
    g = ac.golden()
    meta = json.loads(str(g["meta"]))
    assert meta["conditions"]["exempt_cases"] == 0
    assert any("project_all" in s for s in meta["reference_ran"]) and any("transformBox" in s for s in meta["reference_ran"])
    assert g["vertices"].shape == (300, 3) and g["kp3d"].shape == (9, 3) and g["poses"].shape == (6, 4, 4)
    assert g["t_map"].shape == (40, 80, 64) and 0 < g["t_drawn"].sum() < 40
    what = meta["target_cases"]
    for need in ("clipped left", "clipped right", "clipped top", "clipped bottom", "clipped corner top-left", "outside left",
                 "x <= 0 inside the window", "wide interior", "tall interior"):
        assert need in what


def test_vertex_boxes_equal_the_references_mask_bbox():
    g = ac.golden()
    got = A.vertex_boxes(g["poses"], g["vertices"], g["K"], tuple(g["size"]))
    assert got.dtype == np.int32 and np.array_equal(got, g["mask_bbox"])
    assert (g["mask_bbox"][4, 0] == 1) and (g["mask_bbox"][5, 3] == 479)       # the cut poses reach the strict bounds


def test_vertex_boxes_strict_bounds_and_empty():
    """int(x) == 0 and int(y) == 0 do not count (the reference's ``> 0``), W - 1 and H - 1 do; nothing qualifying
    gives -1 x4; a vertex behind the camera that projects into the image counts, as in the reference."""
    K = np.array([[100.0, 0, 0.0], [0, 100.0, 0.0], [0, 0, 1]])
    pose = np.eye(4)[None]
    pts = lambda uv: np.array([[u / 100.0, v / 100.0, 1.0] for u, v in uv])
    assert A.vertex_boxes(pose, pts([(0.5, 5.5), (5.5, 0.5)]), K, (20, 30)).tolist() == [[-1, -1, -1, -1]]
    assert A.vertex_boxes(pose, pts([(1.5, 2.5), (29.9, 19.9), (30.1, 5), (5, 20.1)]), K, (20, 30)).tolist() == [[1, 29, 2, 19]]
    behind = np.array([[-0.07, -0.05, -1.0]])
    assert A.vertex_boxes(pose, behind, K, (20, 30)).tolist() == [[7, 7, 5, 5]]
    assert A.vertex_boxes(pose, np.array([[0.0, 0.0, 0.0]]), K, (20, 30)).tolist() == [[-1, -1, -1, -1]]


def test_keypoints_equal_the_true_projection_and_the_references_labels():
    g = ac.golden()
    size = tuple(g["size"])
    xy, z, flags = A.project_keypoints(g["poses"], g["kp3d"], g["K"], size)
    want, wz = ac.true_projection(g["poses"], g["kp3d"], g["K"])
    assert np.abs(xy - want).max() <= 1e-9 and np.abs(z - wz).max() <= 1e-12
    inside = (np.floor(want[..., 0] + 0.5) >= 0) & (np.floor(want[..., 0] + 0.5) < size[1]) & \
             (np.floor(want[..., 1] + 0.5) >= 0) & (np.floor(want[..., 1] + 0.5) < size[0])
    assert np.array_equal(flags, np.where(inside, FRONT | IN_IMAGE | SELF | SCENE, FRONT).astype(np.uint8))
    assert not inside.all() and inside.any()
    # the reference's saved labels: its ratios against mask_bbox, undone against the ground-truth box
    vb = A.vertex_boxes(g["poses"], g["vertices"], g["K"], size)
    labels = A.reference_labels(xy, vb, g["gt_bbox"])
    assert np.abs(labels - g["kp_label"]).max() <= 1e-9
    ratios = np.stack([(xy[..., 0] - vb[:, None, 0]) / (vb[:, None, 1] - vb[:, None, 0]),
                       (xy[..., 1] - vb[:, None, 2]) / (vb[:, None, 3] - vb[:, None, 2])], axis=-1)
    assert np.abs(ratios - g["kp_2d"]).max() <= 1e-9 / 50          # (the boxes are at least 50 px wide)
    assert np.abs(labels - xy).max() > 1.0                          # the quirk is real: the labels are not the projections
    assert np.array_equal(g["bbox"], g["gt_bbox"])


def test_kpd_targets_equal_transformbox_and_drawgaussian():
    g = ac.golden()
    out, centres, mask = A.kpd_targets(g["t_part"][:, None, :], g["t_ul"], g["t_br"], want_mask=True)
    assert out.shape == (40, 1, 80, 64) and out.dtype == np.float32
    assert np.array_equal(centres[:, 0], g["t_centre"])
    assert np.array_equal(out[:, 0].view(np.uint32), g["t_map"].view(np.uint32))
    undrawn = ~g["t_drawn"]
    assert not out[undrawn].any() and (centres[undrawn] == -1).all() and (centres[g["t_drawn"]] >= 0).all()
    assert (mask == 1.0).all()
    # the same 40 as one sample of 40 parts per window would not be the same windows: as B = 1 x Kp = 40 with one window
    one = A.kpd_targets(np.repeat(g["t_part"][None, :1], 3, axis=1), g["t_ul"][:1], g["t_br"][:1])[0]
    assert np.array_equal(one[0, 0], out[0, 0]) and np.array_equal(one[0, 2], out[0, 0])


def targets_np(parts, ul, br, in_res, out_res):
    """transformBox + drawGaussian restated in numpy float32 for shapes the fixture does not hold."""
    f = np.float32
    g = A.gaussian_table(1)
    B, Kp = parts.shape[:2]
    out = np.zeros((B, Kp, out_res[0], out_res[1]), np.float32)
    centres = np.full((B, Kp, 2), -1, np.int32)
    for b in range(B):
        for k in range(Kp):
            p = parts[b, k]
            if not (p[0] > 0 and ul[b, 0] < p[0] < br[b, 0] and ul[b, 1] < p[1] < br[b, 1]):
                continue
            c = ((br[b] - f(1)) - ul[b]) / f(2)
            lenH = max(br[b, 1] - ul[b, 1], (br[b, 0] - ul[b, 0]) * f(in_res[0]) / f(in_res[1]))
            lenW = lenH * f(in_res[1]) / f(in_res[0])
            q = p.astype(np.float32) - ul[b]
            q = q + np.maximum(f(0), np.array([(lenW - f(1)) / f(2) - c[0], (lenH - f(1)) / f(2) - c[1]], np.float32))
            q = q * f(out_res[0]) / lenH
            cx, cy = int(round(float(q[0]))), int(round(float(q[1])))
            centres[b, k] = cx, cy
            for y in range(max(0, cy - 3), min(out_res[0], cy + 4)):
                for x in range(max(0, cx - 3), min(out_res[1], cx + 4)):
                    out[b, k, y, x] = g[y - cy + 3, x - cx + 3]
    return out, centres


@pytest.mark.parametrize("res", [(80, 64), (13, 10)])
def test_kpd_targets_other_shapes(res):
    parts, ul, br, in_res, out_res = ac.target_case(*res)
    out, centres = A.kpd_targets(parts, ul, br, in_res, out_res)
    want, wc = targets_np(parts, ul, br, in_res, out_res)
    assert np.array_equal(centres, wc) and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert (wc[:, 4] == -1).all() and (wc[:, :4] >= 0).all()
    # sample 0's window has the map's aspect, so its parts near the window's edges are clipped by the map's borders
    # (the padded windows of samples 1 and 2 leave room on two sides); every entry of the 7 x 7 table is positive
    clipped = [int((out[0, k] > 0).sum()) for k in (1, 2, 3)]
    assert max(clipped) < 49 and (out[0, 0] > 0).sum() == 49


def test_gaussian_table_and_windows():
    g = A.gaussian_table(1)
    assert g.shape == (7, 7) and g.dtype == np.float32 and g[3, 3] == 1.0 and np.array_equal(g, g.T)
    assert A.gaussian_table(2).shape == (13, 13)
    ul, br = A.kpd_windows([[100.7, 50.2, 300.9, 250.1], [5, 5, 635, 475]], [0.5, 0.25], (480, 640))
    # corners truncated to (100, 50, 300, 250), widened by a quarter of 200 x 200 on each side; the second is clamped
    assert ul.dtype == np.float32 and ul.tolist() == [[50.0, 0.0], [0.0, 0.0]] and br.tolist() == [[350.0, 300.0], [639.0, 479.0]]


def test_visibility_of_a_box_seen_head_on():
    v, f, pose, kp = ac.box_case()
    depth, _ = metrics.render_depth(pose, v, f, rc.K, (rc.H, rc.W))
    xy, z, flags = A.project_keypoints(pose, kp, rc.K, (rc.H, rc.W), model_depth=depth)
    seen = FRONT | IN_IMAGE | SELF | SCENE
    hidden = FRONT | IN_IMAGE | SCENE
    want = [seen] * 5 + [hidden] * 9 + [seen, FRONT, 0, 0]
    assert flags[0].tolist() == want
    px = np.floor(xy[0, 14] + 0.5).astype(int)
    assert depth[0, px[1], px[0]] == 0                                  # key point 14 sits on an uncovered pixel
    assert xy[0, 16].tolist() == [-1, -1] and xy[0, 17].tolist() == [-1, -1]
    assert z[0, 16] == pytest.approx(-0.1) and 0 < z[0, 17] < 0.01
    # without a render nothing hides anything; a tolerance larger than the cube hides nothing either
    assert A.project_keypoints(pose, kp, rc.K, (rc.H, rc.W))[2][0].tolist() == [seen] * 15 + [FRONT, 0, 0]
    assert A.project_keypoints(pose, kp, rc.K, (rc.H, rc.W), model_depth=depth, self_tol=0.2)[2][0, :15].tolist() == [seen] * 15


def test_scene_depth_visibility():
    """A plane 0.2 m in front of the camera over the left half, a wall behind the object on the right, two missing rows."""
    v, f, pose, kp = ac.box_case()
    scene = np.full((1, rc.H, rc.W), 1.0, np.float32)
    scene[0, :, :32] = 0.2
    scene[0, 23:25, :] = 0.0
    xy, z, flags = A.project_keypoints(pose, kp[:14], rc.K, (rc.H, rc.W), scene_depth=scene)
    px = np.floor(xy[0] + 0.5).astype(int)
    for k in range(14):
        missing = px[k, 1] in (23, 24)
        left = px[k, 0] < 32
        want = FRONT | IN_IMAGE | SELF | (0 if missing else KNOWN) | (SCENE if missing or not left else 0)
        assert flags[0, k] == want, k
    assert any(px[k, 0] < 32 and px[k, 1] not in (23, 24) for k in range(14)) and any(px[k, 1] in (23, 24) for k in range(14))
    # delta decides: a surface 1 cm in front of a point hides it at delta = 5 mm and not at 15 mm
    near = np.full((1, rc.H, rc.W), np.float32(z[0, 0] - 0.01))
    assert A.project_keypoints(pose, kp[:1], rc.K, (rc.H, rc.W), scene_depth=near, delta=0.005)[2][0, 0] & SCENE == 0
    assert A.project_keypoints(pose, kp[:1], rc.K, (rc.H, rc.W), scene_depth=near, delta=0.015)[2][0, 0] & SCENE
    # two poses sharing one image through scene_index
    two = A.project_keypoints(np.repeat(pose, 2, axis=0), kp[:14], rc.K, (rc.H, rc.W), scene_depth=scene, scene_index=[0, 0])[2]
    assert np.array_equal(two[0], flags[0]) and np.array_equal(two[1], flags[0])


def test_pixel_center_moves_the_pixel():
    """With pixel_center 0.5 the pixel of a projection is floor(u), with 0 it is floor(u + 0.5)."""
    K = np.array([[100.0, 0, 0.0], [0, 100.0, 0.0], [0, 0, 1]])
    pose = np.eye(4)[None]
    kp = np.array([[0.097, 0.05, 1.0]])                                   # u = 9.7, v = 5.0
    depth = np.zeros((1, 12, 12), np.float32)
    depth[0, 5, 10] = 0.5                                                 # hides the point iff its pixel is (10, 5)
    assert A.project_keypoints(pose, kp, K, (12, 12), model_depth=depth)[2][0, 0] & SELF == 0
    assert A.project_keypoints(pose, kp, K, (12, 12), model_depth=depth, pixel_center=0.5)[2][0, 0] & SELF
    # the last pixel: u = 11.4 is in the image (pixel 11), u = 11.6 is not at pixel_center 0 and is at 0.5
    edge = np.array([[0.116, 0.05, 1.0]])
    assert A.project_keypoints(pose, edge, K, (12, 12))[2][0, 0] == FRONT
    assert A.project_keypoints(pose, edge, K, (12, 12), pixel_center=0.5)[2][0, 0] & IN_IMAGE


def test_skew_enters_the_projection():
    K = np.array([[100.0, 7.0, 3.0], [0, 90.0, 4.0], [0, 0, 1]])
    kp = np.array([[0.02, 0.03, 1.0]])
    xy = A.project_keypoints(np.eye(4)[None], kp, K, (50, 50))[0]
    assert xy[0, 0].tolist() == [(100.0 * 0.02 + 7.0 * 0.03) / 1.0 + 3.0, 90.0 * 0.03 / 1.0 + 4.0]


def test_mask_boxes_against_numpy_and_vsd_counts():
    v, f, gt, est, test_u16, index, d = rc.vsd_scene()
    depth, _ = metrics.render_depth(gt, v, f, rc.K, (rc.H, rc.W))
    scene = A.scene_depth_from_u16(test_u16, 0.001)
    assert scene.dtype == np.float32 and np.array_equal(scene, (test_u16.astype(np.float64) * 0.001).astype(np.float32))
    boxes, counts = A.mask_boxes(depth, rc.K, scene, index)
    wb, wc = ac.mask_boxes_np(depth, rc.K, scene, index, metrics.BOP_VSD_DELTA)
    assert np.array_equal(boxes, wb) and np.array_equal(counts, wc)
    vsd_counts = metrics.pose_errors_vsd(gt, gt, v, f, rc.K, test_u16, index, d)[1]
    assert np.array_equal(counts, vsd_counts[:, :2])
    assert (counts[:, 1] < counts[:, 0]).all() and (counts[:, 1] > 0).all()     # the occluder hides a part of every pose
    assert (boxes[:, 1, 0] >= boxes[:, 0, 0]).all() and not np.array_equal(boxes[:, 0], boxes[:, 1])
    # without a scene depth box 1 is box 0
    b0, c0 = A.mask_boxes(depth, rc.K)
    assert np.array_equal(b0[:, 0], boxes[:, 0]) and np.array_equal(b0[:, 1], b0[:, 0]) and np.array_equal(c0[:, 0], c0[:, 1])
    # pixel_center enters the ray lengths only: same covered box, restatement still equal
    b5, c5 = A.mask_boxes(depth, rc.K, scene, index, pixel_center=0.5)
    w5 = ac.mask_boxes_np(depth, rc.K, scene, index, metrics.BOP_VSD_DELTA, 0.5)
    assert np.array_equal(b5, w5[0]) and np.array_equal(c5, w5[1])


def test_mask_boxes_empty_and_single_pixel():
    depth = np.zeros((3, 9, 11), np.float32)
    depth[1, 4, 7] = 1.0
    depth[2, 0, 0] = depth[2, 8, 10] = 2.0
    scene = np.full((1, 9, 11), 0.5, np.float32)                         # everything is hidden behind it
    boxes, counts = A.mask_boxes(depth, np.eye(3), scene, [0, 0, 0])
    assert boxes[0].tolist() == [[-1] * 4, [-1] * 4] and counts[0].tolist() == [0, 0]
    assert boxes[1].tolist() == [[7, 7, 4, 4], [-1] * 4] and counts[1].tolist() == [1, 0]
    assert boxes[2].tolist() == [[0, 10, 0, 8], [-1] * 4] and counts[2].tolist() == [2, 0]


def test_argument_checks():
    v, f, pose, kp = ac.box_case()
    size = (rc.H, rc.W)
    with pytest.raises(ValueError, match="scene index"):
        A.project_keypoints(pose, kp, rc.K, size, scene_depth=np.zeros((1,) + size, np.float32), scene_index=[1])
    with pytest.raises(ValueError, match="scene index"):
        A.mask_boxes(np.zeros((1,) + size, np.float32), rc.K, np.zeros((2,) + size, np.float32), [-1])
    with pytest.raises(ValueError, match="scene_index without"):
        A.project_keypoints(pose, kp, rc.K, size, scene_index=[0])
    with pytest.raises(ValueError, match="float32"):
        A.project_keypoints(pose, kp, rc.K, size, model_depth=np.zeros((1,) + size))
    with pytest.raises(ValueError, match="model_depth has shape"):
        A.project_keypoints(pose, kp, rc.K, size, model_depth=np.zeros((2,) + size, np.float32))
    with pytest.raises(ValueError, match="near"):
        A.project_keypoints(pose, kp, rc.K, size, near=0.0)
    with pytest.raises(ValueError, match="one row per sample"):
        A.kpd_targets(np.zeros((2, 3, 2)), np.zeros((1, 2)), np.zeros((2, 2)))
    with pytest.raises(ValueError, match="uint16"):
        A.scene_depth_from_u16(np.zeros((1, 2, 2), np.int32), 0.001)
    assert A.project_keypoints(np.zeros((0, 3, 4)), kp, rc.K, size)[0].shape == (0, len(kp), 2)
    # the C entry points refuse the same by themselves
    lib = _lib.lib()
    p12 = np.ascontiguousarray(pose.reshape(1, 12))
    Kf = np.ascontiguousarray(rc.K).reshape(9)
    xy, z, fl = np.zeros((len(kp), 2)), np.zeros(len(kp)), np.zeros(len(kp), np.uint8)
    scene, bad = np.zeros(size, np.float32), np.array([1], np.int32)
    rc_ = lib.bp_annotate_keypoints_host(_lib.ptr(p12), 1, _lib.ptr(kp), len(kp), _lib.ptr(Kf), size[0], size[1], 0.0, 0.01, None,
                                         _lib.ptr(scene), 1, _lib.ptr(bad), 0.015, 0.015, _lib.ptr(xy), _lib.ptr(z), _lib.ptr(fl))
    assert rc_ == -1 and b"scene index" in lib.bp_last_error()
    boxes, counts = np.zeros((1, 2, 4), np.int32), np.zeros((1, 2), np.int32)
    rc_ = lib.bp_mask_boxes_host(_lib.ptr(scene), 1, size[0], size[1], _lib.ptr(Kf), 0.0, _lib.ptr(scene), 1, None, 0.015,
                                 _lib.ptr(boxes), _lib.ptr(counts))
    assert rc_ == -1 and b"given together" in lib.bp_last_error()
    assert lib.bp_vertex_boxes_host(None, 1, _lib.ptr(kp), len(kp), _lib.ptr(Kf), 10, 10, _lib.ptr(boxes)) == -1
    g = A.gaussian_table(1)
    assert lib.bp_kpd_targets_host(_lib.ptr(xy), _lib.ptr(scene), _lib.ptr(scene), 1, 1, 320, 256, 80, 64, _lib.ptr(g), 6,
                                   _lib.ptr(scene), _lib.ptr(boxes), None) == -1
    assert b"odd size" in lib.bp_last_error()


def write_tree(base, frames=7):
    """A write_sixd_tree data set of object 1: a 10 cm icosphere mesh (with faces, which the tree's own point-cloud
    writer leaves out), 12 key points on it, `frames` poses in view of LineMod's camera, depth images with a wall, an
    occluder over the left part of the image and a band of missing depth."""
    from PIL import Image
    v, f = rc.icosphere()
    v_mm = v * 50.0
    rng = np.random.default_rng(3)
    kp_mm = v_mm[rng.choice(len(v_mm), 12, replace=False)]
    gt = {}
    for nr in range(frames):
        t = np.array([rng.uniform(-80, 80), rng.uniform(-60, 60), rng.uniform(500, 800)])
        R = rc.rand_rot(rng)
        uv = ac.true_projection(np.hstack([R, t[:, None] / 1000.0])[None], v_mm / 1000.0, synth.CAM_K)[0][0]
        x1, y1 = np.floor(uv.min(axis=0))
        x2, y2 = np.ceil(uv.max(axis=0))
        gt[nr] = [(1, R, t, [x1, y1, x2 - x1, y2 - y1])]
    synth.write_sixd_tree(base, 1, gt, {1: v_mm}, {1: kp_mm}, {1: 100.0})
    with open(os.path.join(base, "models", "obj_01.ply"), "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v_mm), len(f)))
        fh.writelines("%.6f %.6f %.6f\n" % tuple(p) for p in v_mm)
        fh.writelines("3 %d %d %d\n" % tuple(t) for t in f)
    os.makedirs(os.path.join(base, "test", "01", "depth"), exist_ok=True)
    for nr in range(frames):
        d = np.full((480, 640), 1500, np.uint16)
        d[:, :300] = 300
        d[200:204, :] = 0
        Image.fromarray(d).save(os.path.join(base, "test", "01", "depth", "%04d.png" % nr))
    return gt


def test_cli_writes_the_references_layout(tmp_path):
    base, out = str(tmp_path / "sixd"), str(tmp_path / "out") + os.sep
    gt = write_tree(base)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "annotate.py"), "--obj_id", "1", "--sixd_base", base, "--output_base",
                        out, "--total_kp_number", "9", "--train_split", "4", "--visibility", "--depth"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("annotated 7 frames of object 01") and "key points visible per frame" in last and "visib_fract" in last
    d = out + "01"
    for i in range(7):
        kp, bb = np.load(os.path.join(d, "kp_label", "%d.npy" % i)), np.load(os.path.join(d, "bbox", "%d.npy" % i))
        assert kp.shape == (9, 2) and bb.shape == (4,)
        x, y, w, h = gt[i][0][3]
        assert bb.tolist() == [x, y, x + w, y + h]
        line = open(os.path.join(d, "labels", "%04d.txt" % i)).read()
        assert line == "0 %f %f %f %f\n" % ((x + w / 2) / 640, (y + h / 2) / 480, w / 640, h / 480)
    tr, ev = np.load(os.path.join(d, "annot_train.npz")), np.load(os.path.join(d, "annot_eval.npz"))
    assert tr["part"].shape == (4, 9, 2) and ev["part"].shape == (3, 9, 2)
    assert tr["bndbox"].shape == (4, 1, 4) and tr["imgname"].shape == (4, 16) and tr["flags"].shape == (4, 9)
    names = ["".join(chr(c) for c in row) for row in np.concatenate([tr["imgname"], ev["imgname"]])]
    assert sorted(names) == ["%012d.png" % i for i in range(7)]
    for z, rows in ((tr, names[:4]), (ev, names[4:])):
        for j, n in enumerate(rows):
            i = int(n[:-4])
            assert np.array_equal(z["part"][j], np.load(os.path.join(d, "kp_label", "%d.npy" % i)))
            assert np.array_equal(z["bndbox"][j, 0], np.load(os.path.join(d, "bbox", "%d.npy" % i)))
    assert open(os.path.join(d, "train.txt")).read().split() == names[:4]
    # the labels are the true projections of the thinned key points, and the occluder hides some of them
    bench_kp = metrics.refine_keypoints(metrics.load_ply_vertices(os.path.join(base, "kpmodels", "obj_01.ply")), 9) / 1000.0
    pose = np.hstack([gt[0][0][1], np.asarray(gt[0][0][2])[:, None] / 1000.0])[None]
    want = ac.true_projection(pose, bench_kp, synth.CAM_K)[0][0]
    assert np.abs(np.load(os.path.join(d, "kp_label", "0.npy")) - want).max() < 1e-6      # (the tree stores 6 decimals of mm)
    flags = np.concatenate([tr["flags"], ev["flags"]])
    assert ((flags & SELF) == 0).any() and (flags & SELF).any() and (flags & KNOWN).any()


def test_annotate_sequence_reference_labels_and_split(tmp_path):
    from betapose_amd import sixd
    base = str(tmp_path / "sixd")
    gt = write_tree(base, frames=3)
    sys.path.insert(0, ROOT)
    import annotate as cli
    bench, kp3d, faces, size = cli.load_bench(base, 1, 12, True, True)
    assert size == (480, 640) and len(kp3d) == 12
    ann = A.annotate_sequence(bench, 1, kp3d, faces=faces, use_depth=True)
    ref = A.annotate_sequence(bench, 1, kp3d, reference=True)
    assert ann["frames"].tolist() == [0, 1, 2] and set(ref) == {"frames", "bbox", "kp_label", "kp_depth", "kp_flags"}
    vb = A.vertex_boxes(np.array([g[1] for fr in bench.frames for g in fr.gt]), bench.models["01"].vertices, bench.cam, size)
    assert np.array_equal(ref["kp_label"], A.reference_labels(ann["kp_label"], vb, ann["bbox"]))
    assert not np.array_equal(ref["kp_label"], ann["kp_label"])
    assert ann["box_full"].shape == (3, 4) and (ann["visib_fract"] <= 1).all() and (ann["visib_fract"] >= 0).all()
    x_left = ann["box_full"][:, 0] < 300
    assert ((ann["visib_fract"] < 1) == x_left).all()                    # the occluder covers columns below 300
    split = A.write_annotations(str(tmp_path / "o"), ann, 1, seed=5)
    assert len(split["train"]) == 1 and len(split["eval"]) == 2
    assert A.write_annotations(str(tmp_path / "o2"), ann, 1, seed=5) == split
    with pytest.raises(ValueError, match="train_split"):
        A.write_annotations(str(tmp_path / "o3"), ann, 4)
