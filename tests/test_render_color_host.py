"""The host side of the colour renderer (csrc/raster_color_host.cpp through bp_render_color_host, bp_draw_boxes_host,
bp_overlay_host; metrics.render_color, draw_boxes, overlay, load_ply_colored_mesh; betapose_amd/renderer.py): the depth
against render_depth, the shading against an independent numpy ray caster, exact analytic cases, the tie rule,
image_index, accumulation, the box lines, the blend, the Renderer mirror, PLY colours and the argument checks.  No GPU."""
import struct

import numpy as np
import pytest

import raster_common as rc
import render_color_common as cc
from betapose_amd import _lib, metrics

H, W, K = rc.H, rc.W, rc.K


# ---------------------------------------------------------------- 1. the depth is render_depth's
@pytest.mark.parametrize("c", [0.0, 0.5])
@pytest.mark.parametrize("name", ["icosphere", "torus", "box"])
def test_depth_and_skipped_equal_render_depth(name, c):
    color, depth, skipped = cc.host("mesh-%s-%.1f" % (name, c))
    want, want_skipped = rc.host_render(name, c)
    assert color.shape == (4, H, W, 3) and color.dtype == np.uint8 and depth.dtype == np.float32
    assert np.array_equal(depth.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(skipped, want_skipped)
    assert not color[depth == 0].any() and color[depth > 0].any()


@pytest.mark.parametrize("case", ["box_closeup", "half_outside", "outside", "behind_near"])
def test_depth_and_skipped_equal_render_depth_edge_cases(case):
    v, f, pose, near = rc.edge_cases()[case]
    color, depth, skipped = cc.host("edge-" + case)
    want, want_skipped = metrics.render_depth(pose[None], v, f, K, (H, W), near=near)
    assert np.array_equal(depth.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(skipped, want_skipped)
    if case == "behind_near":
        assert skipped[0] > 0
    if case == "outside":
        assert not color.any()


# ---------------------------------------------------------------- 2. the shading against an independent ray caster
@pytest.mark.parametrize("light,c", [(0, 0.0), (1, 0.0), (1, 0.5)])
@pytest.mark.parametrize("name", ["icosphere", "torus", "box"])
def test_shading_matches_numpy_ray_caster(name, light, c):
    """Coverage identical and every channel within 1 level (the u8 rounding boundary under last-bit f64 differences of
    two formulations) on every pixel not within 2^-7 px of a projected edge; at most 5 % of the covered pixels are
    ambiguous and at least 150 are compared (the caps of test_raster_host.check_against_ray_caster)."""
    v, f = rc.MESHES[name]()
    col = cc.colors_for(len(v))
    poses = rc.poses_for(name)
    if light == 1:
        color, depth, _ = cc.host("mesh-%s-%.1f" % (name, c))
    else:
        color, depth, _ = metrics.render_color(poses, v, f, col, K, (H, W), pixel_center=c, light=cc.LIGHTS[0])
    for p in range(4):
        ref, hit = cc.ray_cast_color(poses[p], v, f, col, c, 0.5, cc.LIGHTS[light])
        clear = ~rc.ambiguous(poses[p], v, f, c)
        covered = hit | (depth[p] > 0)
        assert np.array_equal((depth[p] > 0) & clear, hit & clear)
        both = hit & clear
        assert (covered & ~clear).sum() <= 0.05 * covered.sum()
        assert both.sum() >= 150
        diff = np.abs(color[p][both].astype(np.float64) - ref[both])
        print(name, light, c, p, "compared", int(both.sum()), "max diff", diff.max(), "pixels off by one", int((diff > 0).any(1).sum()))
        assert diff.max() <= 1
        assert ref[both].std() > 10                    # a shaded, coloured image, not a constant


# ---------------------------------------------------------------- 3. exact analytic cases
def test_uniform_quad_full_ambient_is_exact():
    color, depth, skipped = cc.host("quad-ambient1")
    want = np.zeros((H, W), bool)
    want[5:15, 10:20] = True
    assert np.array_equal(depth[0] > 0, want) and skipped[0] == 0
    assert np.all(color[0][want] == [200, 100, 50]) and not color[0][~want].any()


def test_quad_lit_from_the_camera_peaks_on_the_optical_axis():
    color, depth, _ = cc.host("quad-on-axis")
    want = np.zeros((H, W), bool)
    want[5:15, 10:20] = True
    assert np.array_equal(depth[0] > 0, want)
    assert tuple(color[0, 9, 14]) == (200, 100, 50)             # light_w = 0.5 + 0.5 * 1
    inside = color[0][want].astype(int)
    assert np.all(inside <= [200, 100, 50]) and np.all(inside >= [100, 50, 25])     # floor(0.5 c + 0.5)
    assert (inside[:, 0] < 200).any()                           # it does fall off away from the axis (cos 0.1 rad: one level)


# ---------------------------------------------------------------- 4. the tie rule
def test_equal_depth_goes_to_the_lowest_face_then_the_lowest_pose():
    red, depth, _ = cc.host("tie-red-blue")
    blue, depth2, _ = cc.host("tie-blue-red")
    drawn = depth[0] > 0
    assert drawn.sum() > 300 and np.array_equal(depth, depth2)
    assert np.all(red[0][drawn] == cc.RED) and np.all(blue[0][drawn] == cc.BLUE)
    two, depth3, skipped = cc.host("tie-two-poses")
    assert np.array_equal(two, red) and np.array_equal(depth3, depth) and len(skipped) == 2


# ---------------------------------------------------------------- 5. image_index
def test_two_poses_in_one_image_is_the_nearer_of_the_two_renders():
    both, depth, skipped = cc.host("index-00")
    single, sdepth, sskipped = cc.host("index-01")
    v, f = rc.torus()
    for p in range(2):
        c1, d1, _ = metrics.render_color(rc.poses_for("torus")[p:p + 1], v, f, cc.colors_for(len(v)), K, (H, W))
        assert np.array_equal(c1[0], single[p]) and np.array_equal(d1[0], sdepth[p])
    a, b = sdepth[0].astype(np.float64), sdepth[1].astype(np.float64)
    a_inf, b_inf = np.where(a > 0, a, np.inf), np.where(b > 0, b, np.inf)
    first = a_inf <= b_inf                                     # ties go to slot 0
    want_depth = np.where(first, sdepth[0], sdepth[1])
    assert np.array_equal(depth[0].view(np.uint32), want_depth.view(np.uint32))
    assert np.array_equal(both[0], np.where(first[..., None], single[0], single[1]))
    assert ((a > 0) & (b > 0) & first).any() and ((a > 0) & (b > 0) & ~first).any()      # each occludes the other somewhere
    assert np.array_equal(skipped, sskipped)


def test_bad_image_index_is_refused_with_a_message():
    v, f = rc.box()
    poses = rc.poses_for("box")[:2]
    col = cc.colors_for(len(v))
    for index, images, text in [([1, 0], 2, "non-decreasing"), ([0, 2], 2, "[0, I)"), ([0, -1], 2, "[0, I)"), (None, 3, "I == P")]:
        with pytest.raises(_lib.BetaposeHipError, match=text.replace("[", r"\[").replace(")", r"\)")):
            metrics.render_color(poses, v, f, col, K, (H, W), image_index=index, images=images)
        with pytest.raises(_lib.BetaposeHipError):
            metrics.draw_boxes(np.zeros((images, H, W, 3), np.uint8), poses, cc.unit_box_corners(), K, image_index=index)


# ---------------------------------------------------------------- 6. accumulation
def test_two_accumulated_meshes_equal_one_render_of_both():
    (sv, sf, sc, ps), (bv, bf, bc, pb), (v, f) = cc.two_mesh_scene()
    c1, d1, k1, c2, d2, k2 = cc.host("accumulate")
    alone = metrics.render_color(pb[None], bv, bf, bc, K, (H, W))
    overlap = (d1[0] > 0) & (alone[1][0] > 0)
    assert overlap.sum() > 20 and not np.any(d1[0][overlap] == alone[1][0][overlap])        # no fragment ties in depth
    assert (alone[1][0] > 0).sum() > overlap.sum()                                        # and the box shows beside it
    want = metrics.render_color(ps[None], v, f, np.concatenate([sc, bc]), K, (H, W))
    assert np.array_equal(c2, want[0]) and np.array_equal(d2.view(np.uint32), want[1].view(np.uint32))
    assert not np.array_equal(c2, c1)


def test_without_accumulate_every_byte_is_written():
    v, f = rc.icosphere()
    poses = np.ascontiguousarray(rc.poses_for("icosphere")[:1, :3, :4])
    col = cc.colors_for(len(v))
    color, depth = np.full((1, H, W, 3), 7, np.uint8), np.full((1, H, W), 7.0, np.float32)
    skipped = np.full(1, 7, np.int32)
    Kf, light = np.ascontiguousarray(K).reshape(9), np.zeros(3)
    p = _lib.ptr
    assert _lib.lib().bp_render_color_host(p(poses), 1, p(v), len(v), p(f), len(f), p(col), None, 1, p(Kf), H, W, 0.0, 0.01,
                                           0.5, p(light), 0, p(color), p(depth), p(skipped)) == 0
    want = metrics.render_color(poses, v, f, col, K, (H, W))
    assert np.array_equal(color, want[0]) and np.array_equal(depth, want[1]) and skipped[0] == 0
    assert not (depth == 7.0).any() and (depth == 0).any()


# ---------------------------------------------------------------- 7. boxes
def raw_draw_boxes(image, poses, corners, colors, c, near, index=None):
    poses = np.ascontiguousarray(np.asarray(poses, np.float64)[:, :3, :4])
    corners = np.ascontiguousarray(corners, np.float64)
    p = _lib.ptr
    _lib.check(_lib.lib().bp_draw_boxes_host(p(poses), len(poses), p(corners), p(colors), index, image.shape[0],
                                             p(np.ascontiguousarray(K).reshape(9)), H, W, c, near, p(image)))


BOX_RGB = metrics.colors_u8(metrics.BOX_CORNER_COLORS)


def test_frontal_box_sets_its_corner_pixels_with_the_corner_colours():
    """The unit box at z = 3 with pixel centres at +0.5: the front face's corners project to the pixel centres (19|43,
    11|35), the back face's to (22.43|39.57, 14.43|31.57)."""
    big, pad = cc.guard_image()
    img = big[pad:pad + 1]
    raw_draw_boxes(img, cc.BOX_POSES["frontal"], cc.unit_box_corners(), BOX_RGB, 0.5, 0.01)
    drawn = (img[0] != 9).any(axis=-1)
    for x, y in [(19, 11), (43, 11), (19, 35), (43, 35), (22, 14), (40, 14), (22, 32), (40, 32)]:
        assert drawn[y, x], (x, y)
    # the front top edge, a horizontal edge from x = 19 to x = 43 on row 11: exactly those columns
    assert np.array_equal(np.flatnonzero(drawn[11]), np.arange(19, 44))
    # corner k = (x: k & 4, z: k & 2, y: k & 1); the front face is z = min
    for k, (x, y) in {0: (19, 11), 1: (19, 35), 4: (43, 11), 5: (43, 35)}.items():
        assert tuple(img[0, y, x]) == tuple(BOX_RGB[k]), k
    assert 150 < drawn.sum() < 400
    assert np.all(big[:pad] == 77) and np.all(big[pad + 1:] == 77)


def test_horizontal_edge_sets_the_columns_its_range_contains():
    """Corners 0, 2, 4, 6 at A and 1, 3, 5, 7 at B: every edge is A-B or a point off the pixel grid (which draws
    nothing), so the image holds the one segment from x = 19.25 to x = 43.25 on row 11: columns 20 .. 43, and its colour
    runs from A's to B's."""
    z = 2.0
    A = [(19.25 - K[0, 2]) / K[0, 0] * z, (11.0 - K[1, 2]) / K[1, 1] * z, z]
    B = [(43.25 - K[0, 2]) / K[0, 0] * z, (11.0 - K[1, 2]) / K[1, 1] * z, z]
    corners = np.array([A, B] * 4)
    colors = np.array([[0, 0, 0], [240, 240, 240]] * 4, np.uint8)
    big, pad = cc.guard_image()
    img = big[pad:pad + 1]
    raw_draw_boxes(img, np.eye(4)[None], corners, colors, 0.0, 0.01)
    drawn = (img[0] != 9).any(axis=-1)
    assert np.array_equal(np.argwhere(drawn), [[11, x] for x in range(20, 44)])
    want = [(240 * (4 * x - 77) + 48) // 96 for x in range(20, 44)]       # a = 256 x - 4928 of dm = 6144, rounded
    assert np.array_equal(img[0, 11, 20:44, 0], want)
    assert np.all(big[:pad] == 77) and np.all(big[pad + 1:] == 77)


def test_edge_crossing_near_is_shortened_and_boxes_out_of_sight_draw_nothing():
    for name, near, some in [("crosses_near", 0.5, True), ("closeup", 0.5, True), ("outside", 0.01, False),
                             ("behind", 0.01, False)]:
        big, pad = cc.guard_image()
        img = big[pad:pad + 1]
        raw_draw_boxes(img, cc.BOX_POSES[name], cc.unit_box_corners(), BOX_RGB, 0.0, near)
        drawn = (img[0] != 9).any(axis=-1)
        assert drawn.any() == some, name
        assert np.all(big[:pad] == 77) and np.all(big[pad + 1:] == 77), name
        if name == "crosses_near":
            # the back face (z = 1.4) lies inside the image, the front corners (z = 0.4) behind near: the four edges
            # between them run from the back corners out to the image border
            X = rc.camera_vertices(cc.BOX_POSES[name][0], cc.unit_box_corners())
            assert (X[:, 2] < near).sum() == 4
            border = np.concatenate([drawn[0], drawn[-1], drawn[:, 0], drawn[:, -1]])
            assert border.sum() >= 4
            assert drawn[:2].sum() >= 4 and drawn[46:].sum() >= 4      # beyond the back face's rows 2 .. 45, both ways


def test_overlapping_boxes_highest_pose_then_edge_wins():
    corners = cc.unit_box_corners()
    pose = cc.BOX_POSES["frontal"]
    base = np.full((1, H, W, 3), 9, np.uint8)
    one = metrics.draw_boxes(base, pose, corners, K)
    green = np.tile(np.array([[0, 255, 0]], np.uint8), (8, 1))
    two = metrics.draw_boxes(one, pose, corners, K, green)
    both = metrics.draw_boxes(base, np.concatenate([pose, pose]), corners, K, image_index=[0, 0])
    drawn = (one[0] != 9).any(axis=-1)
    assert np.all(two[0][drawn] == [0, 255, 0]) and np.array_equal(both, one)
    many = cc.host("boxes-many")[0]
    assert (many[0] != 9).any() and (many[1] != 9).any()
    assert not (cc.host("boxes-nothing")[0] != 9).any()


# ---------------------------------------------------------------- 8. overlay
@pytest.mark.parametrize("alpha", [0, 128, 256])
def test_overlay_is_the_integer_blend(alpha):
    frames, color, depth = cc.overlay_inputs()
    out = cc.host("overlay-%d" % alpha)[0]
    want = (alpha * color.astype(np.int64) + (256 - alpha) * frames.astype(np.int64) + 128) >> 8
    want = np.where((depth > 0)[..., None], want, frames).astype(np.uint8)
    assert np.array_equal(out, want)
    assert np.array_equal(out[depth == 0], frames[depth == 0])
    if alpha == 256:
        assert np.array_equal(out[depth > 0], color[depth > 0])
    if alpha == 0:
        assert np.array_equal(out, frames)


# ---------------------------------------------------------------- 8b. every size-free case on a 113 x 75 image
SIZE = (75, 113)      # W an odd prime above the wave width (raster_common.SIZES)


def check_shading(name, c, color, depth, size):
    """test_shading_matches_numpy_ray_caster's comparison and bars for the four poses of one mesh."""
    v, f = rc.MESHES[name]()
    col = cc.colors_for(len(v))
    poses = rc.poses_for(name, size=size)
    for p in range(4):
        ref, hit = cc.ray_cast_color(poses[p], v, f, col, c, 0.5, cc.LIGHTS[1], size)
        clear = ~rc.ambiguous(poses[p], v, f, c, size=size)
        covered = hit | (depth[p] > 0)
        assert np.array_equal((depth[p] > 0) & clear, hit & clear)
        both = hit & clear
        assert (covered & ~clear).sum() <= 0.05 * covered.sum() and both.sum() >= 150
        diff = np.abs(color[p][both].astype(np.float64) - ref[both])
        print(name, c, p, "compared", int(both.sum()), "max diff", diff.max(), "pixels off by one", int((diff > 0).any(1).sum()))
        assert diff.max() <= 1 and ref[both].std() > 10


@pytest.mark.parametrize("name", cc.SIZE_FREE)
def test_size_free_cases_at_75x113(name):
    """What sections 1 .. 8 assert of a case at 64 x 48, at 113 x 75: the depth and skipped counts are render_depth's,
    the shading the numpy ray caster's, the tie, image_index and accumulation rules, the integer blend; the boxes stay
    inside their image and show where they showed."""
    H, W = SIZE
    K = rc.camera(SIZE)
    out = cc.host(name, SIZE)
    kind, _, rest = name.partition("-")
    if kind == "mesh":
        mesh, c = rest.rsplit("-", 1)
        color, depth, skipped = out
        want, want_skipped = rc.host_render(mesh, float(c), SIZE)
        assert color.shape == (4, H, W, 3) and np.array_equal(depth.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(skipped, want_skipped) and not color[depth == 0].any()
        check_shading(mesh, float(c), color, depth, SIZE)
    elif kind == "edge":
        v, f, pose, near = rc.edge_cases(SIZE)[rest]
        color, depth, skipped = out
        want, want_skipped = metrics.render_depth(pose[None], v, f, K, SIZE, near=near)
        assert np.array_equal(depth.view(np.uint32), want.view(np.uint32)) and np.array_equal(skipped, want_skipped)
        assert not color[depth == 0].any() and color.any() == (rest != "outside")
    elif kind == "tie":
        color, depth, skipped = out
        drawn = depth[0] > 0
        first = cc.BLUE if rest == "blue-red" else cc.RED
        assert drawn.sum() > 300 and np.all(color[0][drawn] == first) and len(skipped) == (2 if rest == "two-poses" else 1)
        assert np.array_equal(depth, cc.host("tie-red-blue", SIZE)[1])
    elif kind == "index":
        single, sdepth, sskipped = cc.host("index-01", SIZE)
        assert np.array_equal(out[2], sskipped)
        a_inf, b_inf = (np.where(d > 0, d, np.inf) for d in sdepth.astype(np.float64))
        first = a_inf <= b_inf
        if rest == "00":
            assert np.array_equal(out[1][0].view(np.uint32), np.where(first, sdepth[0], sdepth[1]).view(np.uint32))
            assert np.array_equal(out[0][0], np.where(first[..., None], single[0], single[1]))
        else:
            v, f = rc.torus()
            for p in range(2):
                c1, d1, _ = metrics.render_color(rc.poses_for("torus", size=SIZE)[p:p + 1], v, f, cc.colors_for(len(v)), K, SIZE)
                assert np.array_equal(c1[0], single[p]) and np.array_equal(d1[0], sdepth[p])
            assert (np.isfinite(a_inf) & np.isfinite(b_inf) & first).any() and (np.isfinite(a_inf) & np.isfinite(b_inf) & ~first).any()
    elif kind == "accumulate":
        (sv, sf, sc, ps), (bv, bf, bc, pb), (v, f) = cc.two_mesh_scene()
        c1, d1, k1, c2, d2, k2 = out
        alone = metrics.render_color(pb[None], bv, bf, bc, K, SIZE)
        overlap = (d1[0] > 0) & (alone[1][0] > 0)
        assert overlap.sum() > 20 and not np.any(d1[0][overlap] == alone[1][0][overlap])    # no fragment ties in depth
        assert (alone[1][0] > 0).sum() > overlap.sum()                                    # and the box shows beside it
        want = metrics.render_color(ps[None], v, f, np.concatenate([sc, bc]), K, SIZE)
        assert np.array_equal(c2, want[0]) and np.array_equal(d2.view(np.uint32), want[1].view(np.uint32))
        assert not np.array_equal(c2, c1)
    elif kind == "boxes":
        drawn = (out[0] != 9).any(axis=-1)
        assert out[0].shape[1:] == (H, W, 3) and drawn.any() == (rest != "nothing")
        if rest == "frontal":                       # 4 edges of 37.5 px, 4 of 26.8, 4 of 5.4: 279 less the shared corners
            assert 200 < drawn.sum() < 320
    else:
        assert kind == "overlay"
        frames, color, depth = cc.overlay_inputs(SIZE)
        alpha = int(rest)
        want = (alpha * color.astype(np.int64) + (256 - alpha) * frames.astype(np.int64) + 128) >> 8
        assert np.array_equal(out[0], np.where((depth > 0)[..., None], want, frames).astype(np.uint8))


# ---------------------------------------------------------------- 9. the Renderer mirror
class _Model:
    def __init__(self, v, f, col_u8):
        self.vertices, self.indices, self.colors = v, f, col_u8.astype(np.float64) / 255.0
        self.bb = metrics.box_corners(v)


def test_renderer_mirrors_the_reference_call_surface():
    from betapose_amd.compat.utils.renderer import Renderer
    from betapose_amd.compat.utils.utils import draw_detections_3D
    from betapose_amd import renderer
    assert Renderer is renderer.Renderer and draw_detections_3D is renderer.draw_detections_3D
    (sv, sf, sc, ps), (bv, bf, bc, pb), (v, f) = cc.two_mesh_scene()
    ren = Renderer((W, H), K)
    rgb, dep = ren.finish()
    assert rgb.shape == (H, W, 3) and rgb.dtype == np.float32 and dep.shape == (H, W) and dep.dtype == np.float32
    assert not rgb.any() and not dep.any()
    ren.draw_model(_Model(sv, sf, sc), np.vstack([ps, [0, 0, 0, 1]]))
    ren.draw_model(_Model(bv, bf, bc), pb)
    rgb, dep = ren.finish()
    want = metrics.render_color(ps[None], v, f, np.concatenate([sc, bc]), K, (H, W), pixel_center=0.5)
    assert np.array_equal(np.round(rgb * 255).astype(np.uint8), want[0][0]) and np.array_equal(dep, want[1][0])
    assert rgb.min() >= 0 and rgb.max() <= 1 and (dep > 0).any()
    assert not rgb[dep == 0].any()
    ren.draw_boundingbox(_Model(bv, bf, bc), pb)
    rgb2, dep2 = ren.finish()
    assert np.array_equal(dep2, dep) and (rgb2 != rgb).any() and (ren.drawn & (dep == 0)).any()
    ren.clear()
    rgb, dep = ren.finish()
    assert not rgb.any() and not dep.any() and not ren.drawn.any()


def test_draw_detections_3d_and_draw_poses():
    from betapose_amd.renderer import draw_detections_3D, draw_poses
    bv, bf = rc.box()
    model = _Model(bv, bf, cc.colors_for(len(bv)))
    image = np.random.default_rng(2).random((H, W, 3)).astype(np.float32)
    pose = np.vstack([cc.BOX_POSES["frontal"][0], [0, 0, 0, 1]])
    assert np.array_equal(draw_detections_3D(image, [], K, {"01": model}, 0.5), image)
    low = [[0, 0.2, 0, 0, 1, 1, pose]]
    assert np.array_equal(draw_detections_3D(image, low, K, {"01": model}, 0.5), image)
    out = draw_detections_3D(image, [[0, 0.9, 0, 0, 1, 1, pose], [0, 0.2, 0, 0, 1, 1, pose]], K, {"01": model}, 0.5)
    changed = (out != image).any(axis=-1)
    lines = (metrics.draw_boxes(np.full((1, H, W, 3), 9, np.uint8), pose[None], model.bb, K, pixel_center=0.5)[0] != 9).any(-1)
    assert np.array_equal(changed, lines) and lines.sum() > 150
    frame = (image * 255).astype(np.uint8)
    drawn = draw_poses(frame, pose[None], model, K, alpha=128)
    col, dep, _ = metrics.render_color(pose[None], bv, bf, metrics.colors_u8(model.colors[:, ::-1]), K, (H, W))
    want = metrics.overlay(frame[None], col, dep, 128)
    want = metrics.draw_boxes(want, pose[None], model.bb, K, BOX_RGB[:, ::-1])
    assert np.array_equal(drawn, want[0]) and (drawn != frame).any()
    assert np.array_equal(draw_poses(frame, pose[None], model, K, alpha=0, box=False), frame)


# ---------------------------------------------------------------- 10. PLY colours
def write_ply(path, fmt, v, f, colors, extra):
    names = ["x", "y", "z"] + (["nx"] if extra else []) + (["red", "green", "blue"] if colors is not None else []) + \
        (["quality"] if extra else [])
    types = {"x": "float", "y": "float", "z": "float", "nx": "double", "red": "uchar", "green": "uchar", "blue": "uchar",
             "quality": "short"}
    head = "ply\nformat %s 1.0\nelement vertex %d\n" % (fmt, len(v))
    head += "".join("property %s %s\n" % (types[n], n) for n in names)
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f)
    rows = []
    for i in range(len(v)):
        row = {"x": v[i, 0], "y": v[i, 1], "z": v[i, 2], "nx": 0.25 * i, "quality": -i}
        if colors is not None:
            row.update(red=int(colors[i, 0]), green=int(colors[i, 1]), blue=int(colors[i, 2]))
        rows.append([row[n] for n in names])
    with open(path, "wb") as out:
        out.write(head.encode())
        if fmt == "ascii":
            for r in rows:
                out.write((" ".join(repr(float(x)) if isinstance(x, float) else str(x) for x in r) + "\n").encode())
            for t in f:
                out.write(("3 %d %d %d\n" % tuple(t)).encode())
            return
        e = "<" if fmt == "binary_little_endian" else ">"
        code = {"float": "f", "double": "d", "uchar": "B", "short": "h"}
        for r in rows:
            out.write(struct.pack(e + "".join(code[types[n]] for n in names), *r))
        for t in f:
            out.write(struct.pack(e + "Biii", 3, *[int(i) for i in t]))


@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_load_ply_colored_mesh(tmp_path, fmt, with_colors, extra):
    v, f = rc.icosphere()
    v = v.astype(np.float32).astype(np.float64)
    colors = cc.colors_for(len(v)) if with_colors else None
    path = str(tmp_path / "mesh.ply")
    write_ply(path, fmt, v, f, colors, extra)
    gv, gf, gc = metrics.load_ply_colored_mesh(path)
    assert np.array_equal(gv, v) and np.array_equal(gf, f) and gf.dtype == np.int32
    assert gc.dtype == np.uint8 and gc.shape == (len(v), 3)
    assert np.array_equal(gc, colors if with_colors else np.full((len(v), 3), 128, np.uint8))
    mv, mf = metrics.load_ply_mesh(path)                         # unchanged: a pair, the same geometry
    assert np.array_equal(mv, v) and np.array_equal(mf, f) and np.array_equal(metrics.load_ply_vertices(path), v)
    m = metrics.Model3D()
    m.load_mesh(path, scale=0.5)
    assert np.array_equal(m.vertices, v * 0.5) and np.array_equal(m.indices, f) and m.bb.shape == (8, 3)
    assert np.allclose(m.colors * 255, gc) and np.array_equal(m.bb[0], m.vertices.min(0)) and np.array_equal(m.bb[7], m.vertices.max(0))
    m.load(path)
    assert np.array_equal(m.vertices, v)


# ---------------------------------------------------------------- 11. argument checks
def test_host_entry_points_refuse_bad_arguments_and_touch_nothing():
    L, p = _lib.lib(), _lib.ptr
    v, f = rc.box()
    col = cc.colors_for(len(v))
    poses = np.ascontiguousarray(rc.poses_for("box")[:2, :3, :4])
    Kf, light = np.ascontiguousarray(K).reshape(9), np.zeros(3)
    color, depth = np.full((2, H, W, 3), 7, np.uint8), np.full((2, H, W), 7.0, np.float32)
    skipped = np.full(2, 7, np.int32)
    index = np.array([0, 1], np.int32)
    bad_faces = f.copy()
    bad_faces[3, 1] = len(v)

    def untouched():
        return (color == 7).all() and (depth == 7.0).all() and (skipped == 7).all()

    good = [p(poses), 2, p(v), len(v), p(f), len(f), p(col), p(index), 2, p(Kf), H, W, 0.0, 0.01, 0.5, p(light), 0, p(color),
            p(depth), p(skipped)]
    changes = [(0, None), (2, None), (4, None), (6, None), (9, None), (15, None), (17, None), (18, None), (19, None), (1, 0), (3, 0),
               (5, 0), (8, 0), (10, 0), (11, -1), (13, 0.0), (7, p(np.array([1, 0], np.int32))), (7, p(np.array([0, 2], np.int32))),
               (7, None, 8, 3), (4, p(bad_faces)), (10, 4097, 11, 4096)]
    for ch in changes:
        args = list(good)
        for i in range(0, len(ch), 2):
            args[ch[i]] = ch[i + 1]
        assert L.bp_render_color_host(*args) < 0 and L.bp_last_error() and untouched(), ch
    # the id overflow: P * F > 2^32 - 2 is refused before anything is read (the arrays are only as large as above)
    args = list(good)
    args[1], args[5], args[7], args[8] = 1 << 16, 1 << 16, None, 1 << 16
    assert L.bp_render_color_host(*args) < 0 and b"2^32 - 2" in L.bp_last_error() and untouched()
    assert L.bp_render_color_host(*good) == 0 and not untouched()

    corners, ccol = cc.unit_box_corners(), BOX_RGB
    color[:] = 7
    good = [p(poses), 2, p(corners), p(ccol), p(index), 2, p(Kf), H, W, 0.0, 0.01, p(color)]
    for ch in [(0, None), (2, None), (3, None), (6, None), (11, None), (1, 0), (5, 0), (7, 0), (8, 0), (10, -1.0),
               (4, p(np.array([1, 0], np.int32))), (4, None, 5, 1), (7, 4097, 8, 4096)]:
        args = list(good)
        for i in range(0, len(ch), 2):
            args[ch[i]] = ch[i + 1]
        assert L.bp_draw_boxes_host(*args) < 0 and L.bp_last_error() and (color == 7).all(), ch
    assert L.bp_draw_boxes_host(*good) == 0 and not (color == 7).all()

    frames, out = np.zeros((2, H, W, 3), np.uint8), np.full((2, H, W, 3), 7, np.uint8)
    good = [p(frames), p(color), p(depth), 2, H, W, 128, p(out)]
    for ch in [(0, None), (1, None), (2, None), (7, None), (3, 0), (4, 0), (5, -2), (6, -1), (6, 257), (4, 4097, 5, 4096)]:
        args = list(good)
        for i in range(0, len(ch), 2):
            args[ch[i]] = ch[i + 1]
        assert L.bp_overlay_host(*args) < 0 and L.bp_last_error() and (out == 7).all(), ch
    assert L.bp_overlay_host(*good) == 0 and not (out == 7).all()


# ---------------------------------------------------------------- the harness's --save_img writer
def test_save_pose_images_writes_one_png_per_solved_frame(tmp_path):
    from PIL import Image
    from betapose_amd import renderer
    bv, bf = rc.box()
    model = _Model(bv, bf, cc.colors_for(len(bv)))
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, size=(3, H, W, 3), dtype=np.uint8)
    indir, outdir = tmp_path / "rgb", tmp_path / "out"
    indir.mkdir()
    for i in range(3):
        Image.fromarray(frames[i]).save(str(indir / ("%04d.png" % i)))
    a, b = cc.BOX_POSES["frontal"][0], cc.BOX_POSES["rotated"][0]
    solved = lambda i, p: {"imgname": "%04d.png" % i, "result": [{}], "cam_R": p[:, :3], "cam_t": p[:, 3:4]}   # noqa: E731
    results = [solved(0, a), {"imgname": "0001.png", "result": [], "cam_R": [], "cam_t": []}, solved(2, b)]
    results[2]["instances"] = [{"cam_R": b[:, :3], "cam_t": b[:, 3:4], "status": 0}, {"cam_R": a[:, :3], "cam_t": a[:, 3:4], "status": 0},
                               {"cam_R": [], "cam_t": [], "status": -1}]
    gt = {0: [{"pose": np.vstack([b, [0, 0, 0, 1]])}]}
    n = renderer.save_pose_images([{"model": model, "results": results, "gt": gt}], str(indir), str(outdir), K,
                                  all_instances=True, batch=2)
    assert n == 2 and sorted(p.name for p in (outdir / "vis").iterdir()) == ["0000.png", "0002.png"]
    got0 = np.asarray(Image.open(str(outdir / "vis" / "0000.png")))
    got2 = np.asarray(Image.open(str(outdir / "vis" / "0002.png")))
    col = metrics.colors_u8(model.colors)
    c0, d0, _ = metrics.render_color(a[None], bv, bf, col, K, (H, W))
    want0 = metrics.draw_boxes(metrics.overlay(frames[:1], c0, d0, 128), a[None], model.bb, K)
    want0 = metrics.draw_boxes(want0, b[None], model.bb, K, renderer.GREEN)
    assert np.array_equal(got0, want0[0])
    c2, d2, _ = metrics.render_color(np.stack([b, a]), bv, bf, col, K, (H, W), image_index=[0, 0])
    want2 = metrics.draw_boxes(metrics.overlay(frames[2:], c2, d2, 128), np.stack([b, a]), model.bb, K, image_index=[0, 0])
    assert np.array_equal(got2, want2[0])
    assert renderer.save_pose_images([{"model": model, "results": results[1:2]}], str(indir), str(tmp_path / "none"), K) == 0
    assert not (tmp_path / "none").exists()
