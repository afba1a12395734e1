"""The host side of the depth rasteriser and VSD (csrc/raster_host.cpp through bp_render_depth_host, metrics.render_depth,
vsd_err, pose_errors_vsd, load_ply_mesh, evaluate_results(faces=..., depth_frames=...)): the host renderer against an
independent ray caster written here, its edge cases and fill rule, the VSD definition on hand-built images, the host
pairing, the harness keys and the mesh loader.  No GPU."""
import os
import struct

import numpy as np
import pytest

import raster_common as rc
from betapose_amd import metrics

H, W, K = rc.H, rc.W, rc.K


def check_against_ray_caster(depth, pose, v, f, c, min_compared=150, size=rc.SIZE):
    """Coverage identical and depth equal to 1e-6 relative on every pixel that is not within 2^-7 px of a projected edge;
    at most 5 % of the covered pixels may be ambiguous and at least ``min_compared`` covered pixels must be compared."""
    ref = rc.ray_cast(pose, v, f, c, size)
    amb = rc.ambiguous(pose, v, f, c, size=size)
    covered = (ref > 0) | (depth > 0)
    clear = ~amb
    assert np.array_equal((depth > 0) & clear, (ref > 0) & clear)
    both = (ref > 0) & clear
    n_amb, n_cmp = int((amb & covered).sum()), int(both.sum())
    assert n_amb <= 0.05 * covered.sum(), (n_amb, int(covered.sum()))
    assert n_cmp >= min_compared, n_cmp
    rel = np.abs(depth[both].astype(np.float64) - ref[both]) / ref[both]
    assert rel.max() <= 1e-6, rel.max()


@pytest.mark.parametrize("c", [0.0, 0.5])
@pytest.mark.parametrize("name", ["icosphere", "torus", "box"])
def test_host_render_matches_ray_caster(name, c):
    v, f = rc.MESHES[name]()
    poses = rc.poses_for(name)
    depth, skipped = rc.host_render(name, c)
    assert depth.shape == (4, H, W) and depth.dtype == np.float32 and not skipped.any()
    for p in range(4):
        check_against_ray_caster(depth[p], poses[p], v, f, c)


def test_pixel_center_shifts_the_image():
    """The two conventions differ: the same pose drawn at c = 0 and c = 0.5 is not the same image."""
    assert not np.array_equal(rc.host_render("icosphere", 0.0)[0], rc.host_render("icosphere", 0.5)[0])


def test_box_closeup_covers_the_frame():
    v, f, pose, near = rc.edge_cases()["box_closeup"]
    depth, skipped = metrics.render_depth(pose[None], v, f, K, (H, W), near=near)
    assert skipped[0] == 0
    assert (depth[0] > 0).mean() > 0.9
    check_against_ray_caster(depth[0], pose, v, f, 0.0)


def test_object_half_outside_the_frame():
    v, f, pose, near = rc.edge_cases()["half_outside"]
    depth, skipped = metrics.render_depth(pose[None], v, f, K, (H, W), near=near)
    assert skipped[0] == 0
    assert (depth[0][:, 0] > 0).any() and not (depth[0][:, W // 2:] > 0).any()
    check_against_ray_caster(depth[0], pose, v, f, 0.0, min_compared=100)


def test_object_outside_the_frame_draws_nothing():
    v, f, pose, near = rc.edge_cases()["outside"]
    depth, skipped = metrics.render_depth(pose[None], v, f, K, (H, W), near=near)
    assert skipped[0] == 0 and not depth.any()


def test_vertices_behind_near_are_skipped_and_counted():
    v, f, pose, near = rc.edge_cases()["behind_near"]
    X = rc.camera_vertices(pose, v)
    behind = (X[f][:, :, 2] < near).any(axis=1)
    assert 0 < behind.sum() < len(f)
    depth, skipped = metrics.render_depth(pose[None], v, f, K, (H, W), near=near)
    assert skipped[0] == behind.sum()
    assert np.isfinite(depth).all() and (depth >= 0).all()
    drawn = depth[depth > 0]
    assert len(drawn) and drawn.min() >= near and drawn.max() <= X[:, 2].max()


# ---------------------------------------------------------------- the other image sizes (raster_common.SIZES)

NEW_SIZES = rc.SIZES[1:]


def size_id(size):
    return "%dx%d" % tuple(size)


@pytest.mark.parametrize("c", [0.0, 0.5])
@pytest.mark.parametrize("name", ["icosphere", "torus", "box"])
@pytest.mark.parametrize("size", NEW_SIZES, ids=size_id)
def test_host_render_matches_ray_caster_at_size(size, name, c):
    """test_host_render_matches_ray_caster on an image whose width is no multiple of anything and on one higher than
    wide, with the same bars."""
    v, f = rc.MESHES[name]()
    poses = rc.poses_for(name, size=size)
    depth, skipped = rc.host_render(name, c, size)
    assert depth.shape == (4,) + tuple(size) and depth.dtype == np.float32 and not skipped.any()
    for p in range(4):
        check_against_ray_caster(depth[p], poses[p], v, f, c, size=size)


@pytest.mark.parametrize("case,min_compared", [("box_closeup", 150), ("half_outside", 100), ("behind_near", 0)])
@pytest.mark.parametrize("size", NEW_SIZES, ids=size_id)
def test_edge_cases_at_size(size, case, min_compared):
    """The close-up, the object half outside and the cube across the camera plane at the other sizes: what the tests
    above assert of each at 48 x 64, the first two against the ray caster."""
    H, W = size
    v, f, pose, near = rc.edge_cases(size)[case]
    depth, skipped = metrics.render_depth(pose[None], v, f, rc.camera(size), size, near=near)
    if case == "behind_near":
        X = rc.camera_vertices(pose, v)
        behind = (X[f][:, :, 2] < near).any(axis=1)
        assert 0 < behind.sum() < len(f) and skipped[0] == behind.sum()
        assert np.isfinite(depth).all() and (depth >= 0).all()
        drawn = depth[depth > 0]
        assert len(drawn) and drawn.min() >= near and drawn.max() <= X[:, 2].max()
        return
    assert skipped[0] == 0
    if case == "box_closeup":
        assert (depth[0] > 0).mean() > 0.9
    else:
        assert (depth[0][:, 0] > 0).any() and not (depth[0][:, W // 2:] > 0).any()
    check_against_ray_caster(depth[0], pose, v, f, 0.0, min_compared, size)


def test_large_coordinates_need_64_bit_edge_functions():
    """raster_common.big_quad: vertices 10 000 .. 16 000 px from the origin, edge products of about 2^44, the diagonal
    across the 113 x 75 image.  Coverage and depth against the ray caster with the usual bars; both triangles own pixels."""
    size = rc.BIG_QUAD_SIZE
    v, f = rc.big_quad()
    uv = v[:, :2] / v[:, 2:] * rc.camera(size)[0, 0] + rc.camera(size)[[0, 1], 2]
    assert np.abs(uv).min() >= 10000 and np.abs(uv).max() <= 16000
    snapped = np.rint(uv * 256).astype(np.int64)
    worst = max(abs(int((b - a)[0]) * int((c - a)[1])) for a in snapped for b in snapped for c in snapped)
    assert worst > 2 ** 43                      # what an edge function multiplies here does not fit in 32 (or 40) bits
    pose = np.eye(4)[:3]
    depth, skipped = metrics.render_depth(pose[None], v, f, rc.camera(size), size)
    assert skipped[0] == 0 and (depth[0] > 0).all()
    check_against_ray_caster(depth[0], pose, v, f, 0.0, size=size)
    for tri in f:                               # each triangle alone draws its side of the diagonal
        one = metrics.render_depth(pose[None], v, tri[None], rc.camera(size), size)[0][0] > 0
        assert 1000 < one.sum() < one.size - 1000


def test_vertex_past_the_projection_range_skips_its_triangles():
    """The same quad with the shared corner 2 at u = 16 390 px, past RS_MAX_UV = 16 384: both triangles are skipped and
    counted, nothing is drawn; at u = 16 380 px they are drawn."""
    size = rc.BIG_QUAD_SIZE
    v, f = rc.big_quad(out_of_range=True)
    pose = np.eye(4)[None, :3]
    depth, skipped = metrics.render_depth(pose, v, f, rc.camera(size), size)
    assert skipped[0] == 2 and not depth.any()
    corners = list(rc.BIG_QUAD_CORNERS)
    corners[2] = (16380.0, corners[2][1])
    v, f = rc.pixel_quad(corners, rc.BIG_QUAD_DEPTHS, size)
    depth, skipped = metrics.render_depth(pose, v, f, rc.camera(size), size)
    assert skipped[0] == 0 and (depth[0] > 0).all()


@pytest.mark.parametrize("faces", [[[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 3, 2]], [[0, 1, 3], [1, 2, 3]], [[3, 1, 0], [1, 3, 2]]])
@pytest.mark.parametrize("c", [0.0, 0.5])
def test_shared_edge_and_top_left_rule(faces, c):
    """Two coplanar triangles that form the rectangle [10, 20] x [5, 15] in pixel-centre coordinates, either diagonal and
    either winding: the pixel centres ON its left and top edges are drawn, those on its right and bottom edges are not,
    and the shared diagonal leaves no hole -- exactly the pixels 10 .. 19 x 5 .. 14."""
    z = 2.0
    corners = [(10, 5), (20, 5), (20, 15), (10, 15)]
    v = np.array([[(u + c - K[0, 2]) / K[0, 0] * z, (w + c - K[1, 2]) / K[1, 1] * z, z] for u, w in corners])
    depth, skipped = metrics.render_depth(np.eye(4)[None, :3], v, np.array(faces, np.int32), K, (H, W), pixel_center=c)
    want = np.zeros((H, W), bool)
    want[5:15, 10:20] = True
    assert np.array_equal(depth[0] > 0, want)
    assert np.all(depth[0][want] == np.float32(z)) and skipped[0] == 0


def test_render_depth_rejects_bad_arguments():
    v, f = rc.box()
    pose = np.eye(4)[None, :3].copy()
    pose[0, 2, 3] = 3.0
    bad = f.copy()
    bad[3, 1] = len(v)
    with pytest.raises(ValueError):
        metrics.render_depth(pose, v, bad, K, (H, W))
    from betapose_amd import _lib
    L = _lib.lib()
    depth, skipped = np.zeros((1, H, W), np.float32), np.zeros(1, np.int32)
    Kf = np.ascontiguousarray(K).reshape(9)
    p = _lib.ptr
    good = [p(pose), 1, p(v), len(v), p(f), len(f), p(Kf), H, W, 0.0, 0.01, p(depth), p(skipped)]
    assert L.bp_render_depth_host(*good) == 0
    for i, val in [(0, None), (2, None), (4, None), (6, None), (11, None), (12, None), (1, 0), (3, 0), (5, 0), (7, 0), (8, -1),
                   (10, 0.0)]:
        args = list(good)
        args[i] = val
        assert L.bp_render_depth_host(*args) < 0, i
    args = list(good)
    args[7], args[8] = 4097, 4096           # H * W > 2^24 (refused before anything is touched)
    assert L.bp_render_depth_host(*args) < 0
    args = list(good)
    args[4] = p(bad)
    assert L.bp_render_depth_host(*args) < 0 and b"face index" in L.bp_last_error()


# ---------------------------------------------------------------- VSD definition

KV = np.array([[100.0, 0.0, 1.5], [0.0, 100.0, 1.5], [0.0, 0.0, 1.0]])   # rays within 1.0003 of the axis: dist ~ depth
TAUS = (0.2, 0.4)
DIAM = 0.1


def test_vsd_identical_renders_give_zero():
    gt = np.zeros((4, 4))
    gt[1:3, 1:4] = 1.0
    # test image = the surface itself: every rendered pixel is visible in both masks, every distance is 0 -> 0 / 6
    assert np.array_equal(metrics.vsd_err(gt, gt, gt, KV, 0.015, TAUS, DIAM), [0.0, 0.0])
    assert np.array_equal(metrics.vsd_err(gt, gt, gt, KV, 0.015, metrics.BOP_VSD_TAUS, DIAM), np.zeros(10))


def test_vsd_disjoint_masks_give_one():
    gt, est = np.zeros((4, 4)), np.zeros((4, 4))
    gt[:, :2], est[:, 2:] = 1.0, 1.0
    # no test depth anywhere: both renders fully visible, 8 + 8 pixels, no intersection -> (0 + 16) / 16
    assert np.array_equal(metrics.vsd_err(np.zeros((4, 4)), gt, est, KV, 0.015, TAUS, DIAM), [1.0, 1.0])


def test_vsd_partial_overlap_counts_the_complement():
    gt, est = np.zeros((4, 4)), np.zeros((4, 4))
    gt[0, :], est[0, 1:], est[1, 0] = 1.0, 1.0, 1.0
    # gt 4 px, est 4 px, 3 shared at equal distance: inter 3, union 5 -> (0 + 2) / 5 for every tau
    assert np.array_equal(metrics.vsd_err(np.zeros((4, 4)), gt, est, KV, 0.015, TAUS, DIAM), [0.4, 0.4])


def test_vsd_occluder_removes_pixels_from_both_masks():
    gt = np.zeros((4, 4))
    gt[:2, :] = 1.0                                     # 8 rendered pixels at 1.0
    est = np.where(gt > 0, gt + 0.03, 0.0)              # the estimate 0.3 diameters behind
    test = gt.copy()
    test[:2, :2] = 0.5                                  # an occluder half a metre in front of four of them
    # occluded four: dist_gt - dist_test = 0.5 > delta and dist_est - dist_test > delta -> in neither mask.
    # the other four: the ground truth is visible (difference 0); the estimate is 0.03 > delta behind the test surface,
    # so its own clause fails, but it is rendered where the ground truth is visible -> visible.  inter = union = 4,
    # |dist_gt - dist_est| / diameter = 0.3: >= 0.2 on all four -> 4 / 4; < 0.4 -> 0 / 4
    assert np.array_equal(metrics.vsd_err(test, gt, est, KV, 0.015, TAUS, DIAM), [1.0, 0.0])
    m = metrics.vsd_masks(test, gt, est, KV, 0.015)
    assert m["visib_gt"].sum() == 4 and m["union"].sum() == 4 and not m["visib_gt"][:2, :2].any()
    # without the occluder all eight count
    assert metrics.vsd_masks(gt, gt, est, KV, 0.015)["inter"].sum() == 8


def test_vsd_empty_union_gives_one():
    z = np.zeros((4, 4))
    assert np.array_equal(metrics.vsd_err(z, z, z, KV, 0.015, TAUS, DIAM), [1.0, 1.0])
    gt = np.zeros((4, 4))
    gt[1, 1] = 1.0
    test = np.full((4, 4), 0.5)                         # everything rendered is hidden behind the test surface
    assert np.array_equal(metrics.vsd_err(test, gt, gt, KV, 0.015, TAUS, DIAM), [1.0, 1.0])


def test_vsd_distance_is_not_depth():
    """Off the axis a depth becomes a longer distance: a depth difference just under delta on the axis exceeds it there."""
    Kw = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])     # pixel (3, 0): ray (3, 0, 1), length sqrt(10)
    gt, test = np.zeros((1, 4)), np.zeros((1, 4))
    gt[0, 0], gt[0, 3], test[0, 0], test[0, 3] = 1.01, 1.01, 1.0, 1.0
    m = metrics.vsd_masks(test, gt, gt, Kw, 0.015)
    assert m["visib_gt"][0, 0] and not m["visib_gt"][0, 3]                  # 0.01 <= 0.015 < 0.01 * sqrt(10)
    assert m["dist_gt"][0, 3] == 1.01 * np.sqrt(10.0)


def test_bop_vsd_constants():
    assert np.allclose(metrics.BOP_VSD_TAUS, np.arange(1, 11) * 0.05) and len(metrics.BOP_VSD_TAUS) == 10
    assert np.allclose(metrics.BOP_VSD_THETAS, np.arange(1, 11) * 0.05) and metrics.BOP_VSD_DELTA == 0.015


# ---------------------------------------------------------------- host pairing

def test_pose_errors_vsd_host_is_render_plus_vsd_err():
    v, f, gt, est, test, index, d = rc.vsd_scene()
    err, counts = metrics.pose_errors_vsd(gt, est, v, f, K, test, index, d)
    assert err.shape == (5, 10) and counts.shape == (5, 4) and counts.dtype == np.int32
    dg = metrics.render_depth(gt, v, f, K, (H, W))[0]
    de = metrics.render_depth(est, v, f, K, (H, W))[0]
    for p in range(5):
        t = test[index[p]].astype(np.float64) * 0.001
        want = metrics.vsd_err(t, dg[p], de[p], K, metrics.BOP_VSD_DELTA, metrics.BOP_VSD_TAUS, d)
        assert np.array_equal(err[p], want)
        assert counts[p, 0] == (dg[p] > 0).sum()
    rendered, visib, inter, union = counts.T
    assert (inter <= union).all() and (visib <= rendered).all() and (visib <= union).all() and (rendered > 150).all()
    assert (visib < rendered).all()                     # the occluder plane hides a part of every ground truth
    assert 0.0 < err.min() and err.max() <= 1.0 and (np.diff(err, axis=1) <= 0).all()   # a looser tau never scores worse
    with pytest.raises(ValueError):
        metrics.pose_errors_vsd(gt, est, v, f, K, test, index + 1, d)
    with pytest.raises(ValueError):
        metrics.pose_errors_vsd(gt, est, v, f, K, test.astype(np.int32), index, d)
    with pytest.raises(ValueError):
        metrics.pose_errors_vsd(gt, est, v, f, K, test, index, d, taus=np.linspace(0.01, 0.5, 17))


# ---------------------------------------------------------------- harness

def _harness_inputs(shift):
    v, f = rc.torus()
    v = v * (0.1 / rc.diameter(v))
    d = rc.diameter(v)
    rng = np.random.default_rng(31)
    final, gt_frames, depth_frames = [], {}, {}
    for nr in range(3):
        pose = np.eye(4)
        pose[:3, :3] = rc.rand_rot(rng)
        pose[:3, 3] = [0.0, 0.0, d * rng.uniform(2.2, 2.6)]
        depth = metrics.render_depth(pose[None], v, f, K, (H, W))[0][0]
        depth_frames[nr] = np.round(depth.astype(np.float64) * 1000.0).astype(np.uint16)
        gt_frames[nr] = [{"pose": pose, "bbox": [10, 5, 40, 35]}]
        final.append({"imgname": "%04d.png" % nr, "result": [{"bbox": np.array([10.0, 5.0, 50.0, 40.0])}],
                      "cam_R": pose[:3, :3].copy(), "cam_t": (pose[:3, 3] + [shift * d, 0.0, 0.0]).reshape(3, 1)})
    return final, gt_frames, depth_frames, v, f, d


def test_evaluate_results_vsd_keys():
    final, gt_frames, depth_frames, v, f, d = _harness_inputs(0.0)
    base = metrics.evaluate_results(final, gt_frames, v, K, d * 1000.0)
    assert set(base) == {"mean_add", "mean_2d_acc", "mean_iou", "mean_add_err_mm", "n"}
    assert set(metrics.evaluate_results(final, gt_frames, v, K, d * 1000.0, faces=f)) == set(base)         # both are needed
    m = metrics.evaluate_results(final, gt_frames, v, K, d * 1000.0, faces=f, depth_frames=depth_frames)
    assert set(m) == set(base) | {"ar_vsd", "mean_vsd_err", "mean_visib_fract"}
    assert {k: m[k] for k in base} == base
    # est = gt, the test images are the ground truth's own renders (to the millimetre): every error is 0
    assert m["ar_vsd"] == 1.0 and m["mean_vsd_err"] == 0.0 and m["mean_visib_fract"] == 1.0


def test_evaluate_results_vsd_far_estimates():
    final, gt_frames, depth_frames, v, f, d = _harness_inputs(1.0)       # one diameter sideways: the masks are disjoint
    m = metrics.evaluate_results(final, gt_frames, v, K, d * 1000.0, faces=f, depth_frames=depth_frames)
    assert m["ar_vsd"] == 0.0 and m["mean_vsd_err"] > 0.95 and m["mean_visib_fract"] == 1.0
    del depth_frames[1]
    with pytest.raises(KeyError):
        metrics.evaluate_results(final, gt_frames, v, K, d * 1000.0, faces=f, depth_frames=depth_frames)


# ---------------------------------------------------------------- mesh loading

QUAD_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]], dtype=np.float64)
QUAD_F = [[0, 1, 2, 3], [0, 1, 4], [1, 2, 4], [4, 2, 3, 0, 1]]
QUAD_TRIS = [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [4, 2, 3], [4, 3, 0], [4, 0, 1]]


def test_load_ply_mesh_ascii(tmp_path):
    path = os.path.join(tmp_path, "m.ply")
    with open(path, "w") as fh:
        fh.write("ply\nformat ascii 1.0\ncomment made by the test\nelement vertex 5\nproperty float x\nproperty float y\n"
                 "property float z\nproperty uchar red\nelement face 4\nproperty list uchar int vertex_indices\nend_header\n")
        for p in QUAD_V:
            fh.write("%r %r %r 7\n" % tuple(float(x) for x in p))
        for poly in QUAD_F:
            fh.write("%d %s\n" % (len(poly), " ".join(map(str, poly))))
    v, f = metrics.load_ply_mesh(path)
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert np.array_equal(v, QUAD_V) and f.tolist() == QUAD_TRIS
    assert np.array_equal(metrics.load_ply_vertices(path), v)


def test_load_ply_mesh_binary(tmp_path):
    path = os.path.join(tmp_path, "m.ply")
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty double x\nproperty double y\n"
                 b"property double z\nelement face 4\nproperty uchar flag\nproperty list uchar uint vertex_index\nend_header\n")
        for p in QUAD_V:
            fh.write(struct.pack("<3d", *p))
        for poly in QUAD_F:
            fh.write(struct.pack("<BB%dI" % len(poly), 9, len(poly), *poly))
    v, f = metrics.load_ply_mesh(path)
    assert np.array_equal(v, QUAD_V) and f.tolist() == QUAD_TRIS
    assert np.array_equal(metrics.load_ply_vertices(path), v)
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\n"
                 b"property float z\nend_header\n" + struct.pack("<3f", 1, 2, 3))
    with pytest.raises(ValueError):
        metrics.load_ply_mesh(path)                     # no face element


# ---------------------------------------------------------------- depth frames of a SIXD tree

def test_load_sixd_depth_is_opt_in(tmp_path):
    yaml = pytest.importorskip("yaml")
    from PIL import Image
    from betapose_amd import sixd
    base = str(tmp_path)
    seq = os.path.join(base, "test", "02")
    os.makedirs(os.path.join(seq, "depth"))
    os.makedirs(os.path.join(base, "models"))
    with open(os.path.join(base, "models", "models_info.yml"), "w") as fh:
        yaml.safe_dump({1: {"diameter": 100.0}}, fh)
    entry = {"cam_R_m2c": np.eye(3).reshape(-1).tolist(), "cam_t_m2c": [0.0, 0.0, 500.0], "obj_bb": [1, 2, 3, 4], "obj_id": 1}
    with open(os.path.join(seq, "gt.yml"), "w") as fh:
        yaml.safe_dump({0: [entry], 1: [entry]}, fh)
    with open(os.path.join(seq, "info.yml"), "w") as fh:
        yaml.safe_dump({0: {}, 1: {}}, fh)
    images = [np.arange(12, dtype=np.uint16).reshape(3, 4) * 5000 + k for k in range(2)]    # values beyond 8 and 15 bits
    for k, im in enumerate(images):
        Image.fromarray(im).save(os.path.join(seq, "depth", "%04d.png" % k))
    bench = sixd.load_sixd(base, 2)
    assert all(fr.depth is None for fr in bench.frames)
    bench = sixd.load_sixd(base, 2, load_depth=True)
    for fr, im in zip(bench.frames, images):
        assert fr.depth.dtype == np.uint16 and np.array_equal(fr.depth, im)
    Image.fromarray(np.zeros((3, 4), np.uint8)).save(os.path.join(seq, "depth", "0001.png"))
    with pytest.raises(ValueError):
        sixd.load_sixd(base, 2, load_depth=True)
