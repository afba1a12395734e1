"""Textured meshes on the host: the PLY and PNG loaders, the mip pyramid, and
metrics.render_color(uv=, texture=) through bp_render_color_textured_host against the numpy restatement of
texture_common.py, against the vertex-colour path where the two must agree, and through the synthesiser.  No GPU."""
import struct

import numpy as np
import pytest

import raster_common as rc
import texture_common as tc
from betapose_amd import _lib, metrics, synth


# ------------------------------------------------------------------------------------------------------------ 1. loader
# a quad and a triangle that share an edge; every coordinate is a multiple of 1/8, exact in float32 and in decimal
PLY_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0], [2, 0.5, 0.25]], np.float64)
PLY_UV = np.array([[0.0, 0.0], [0.5, 0.125], [0.625, 0.875], [0.125, 1.0], [1.0, 0.5]])
PLY_POLYS = [[0, 1, 2, 3], [1, 4, 2]]
PLY_FACES = np.array([[0, 1, 2], [0, 2, 3], [1, 4, 2]], np.int32)
PLY_RGB = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 8, 7], [100, 150, 200]], np.uint8)
# per-corner coordinates that differ from the per-vertex ones at the shared vertices: a seam
PLY_CORNERS = [[(0.0, 0.0), (0.5, 0.125), (0.625, 0.875), (0.125, 1.0)], [(0.25, 0.25), (0.75, 0.5), (0.375, 0.625)]]
PLY_CORNER_UV = np.array([[PLY_CORNERS[0][0], PLY_CORNERS[0][1], PLY_CORNERS[0][2]],
                          [PLY_CORNERS[0][0], PLY_CORNERS[0][2], PLY_CORNERS[0][3]],
                          [PLY_CORNERS[1][0], PLY_CORNERS[1][1], PLY_CORNERS[1][2]]])
FORMATS = ["ascii", "binary_little_endian", "binary_big_endian"]


def write_ply(path, fmt, layout, colors=False, texture_file=None, uv_names=("texture_u", "texture_v")):
    """layout: "vertex" (scalar vertex properties), "face" (a texcoord list), "both" or None."""
    per_vertex, per_face = layout in ("vertex", "both"), layout in ("face", "both")
    head = ["ply", "format %s 1.0" % fmt, "comment made for a test"]
    if texture_file:
        head += ["comment TextureFile %s" % texture_file, "comment TextureFile ignored.png"]
    head += ["element vertex %d" % len(PLY_V), "property float x", "property float y", "property float z"]
    if colors:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    if per_vertex:
        head += ["property float %s" % uv_names[0], "property float %s" % uv_names[1]]
    head += ["element face %d" % len(PLY_POLYS), "property list uchar int vertex_indices"]
    if per_face:
        head += ["property list uchar float texcoord"]
    head += ["end_header"]
    # in the "both" layout the vertex properties hold other numbers: the face list must win
    vertex_uv = PLY_UV if layout == "vertex" else PLY_UV[::-1]
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode())
        e = "<" if fmt == "binary_little_endian" else ">"
        for i in range(len(PLY_V)):
            if fmt == "ascii":
                row = ["%r" % float(t) for t in PLY_V[i]] + (["%d" % t for t in PLY_RGB[i]] if colors else []) + \
                      (["%r" % float(t) for t in vertex_uv[i]] if per_vertex else [])
                out.write((" ".join(row) + "\n").encode())
            else:
                out.write(struct.pack(e + "3f", *PLY_V[i]) + (bytes(PLY_RGB[i].tolist()) if colors else b"") +
                          (struct.pack(e + "2f", *vertex_uv[i]) if per_vertex else b""))
        for poly, corners in zip(PLY_POLYS, PLY_CORNERS):
            flat = [t for corner in corners for t in corner]
            if fmt == "ascii":
                row = ["%d" % len(poly)] + ["%d" % i for i in poly] + (["%d" % len(flat)] + ["%r" % t for t in flat] if per_face else [])
                out.write((" ".join(row) + "\n").encode())
            else:
                out.write(struct.pack(e + "B%di" % len(poly), len(poly), *poly) +
                          (struct.pack(e + "B%df" % len(flat), len(flat), *flat) if per_face else b""))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("layout", ["vertex", "face", "both", None])
def test_loader_reads_both_layouts_in_every_format(tmp_path, fmt, layout):
    """Per-vertex coordinates are copied to the corners, a per-face list is carried along the fan (0, k, k + 1), the face
    list wins where a file has both, a file without either gives None; and the older loaders return what they did."""
    path = str(tmp_path / "m.ply")
    write_ply(path, fmt, layout, colors=layout != "face")
    v, f, col, uv, texture_file = metrics.load_ply_textured_mesh(path)
    assert np.array_equal(v, PLY_V) and np.array_equal(f, PLY_FACES) and f.dtype == np.int32
    assert texture_file is None
    if layout is None:
        assert uv is None
    else:
        assert uv.dtype == np.float64 and uv.shape == (3, 3, 2)
        assert np.array_equal(uv, PLY_UV[PLY_FACES] if layout == "vertex" else PLY_CORNER_UV)
    want_col = PLY_RGB if layout != "face" else np.full((5, 3), 128, np.uint8)
    assert np.array_equal(col, want_col)
    # the three older loaders: the same vertices, faces and colours (or the grey) as before
    v3, f3, c3 = metrics.load_ply_colored_mesh(path)
    assert np.array_equal(v3, PLY_V) and np.array_equal(f3, PLY_FACES) and np.array_equal(c3, want_col) and c3.dtype == np.uint8
    v2, f2 = metrics.load_ply_mesh(path)
    assert np.array_equal(v2, PLY_V) and np.array_equal(f2, PLY_FACES)
    assert np.array_equal(metrics.load_ply_vertices(path), PLY_V)


@pytest.mark.parametrize("names", [("u", "v"), ("s", "t")])
def test_loader_reads_the_other_vertex_property_names(tmp_path, names):
    path = str(tmp_path / "m.ply")
    write_ply(path, "ascii", "vertex", uv_names=names)
    assert np.array_equal(metrics.load_ply_textured_mesh(path)[3], PLY_UV[PLY_FACES])


def test_texture_file_is_resolved_against_the_plys_folder(tmp_path):
    (tmp_path / "sub").mkdir()
    path = str(tmp_path / "sub" / "m.ply")
    write_ply(path, "binary_little_endian", "vertex", texture_file="obj_000001.png")
    assert metrics.load_ply_textured_mesh(path)[4] == str(tmp_path / "sub" / "obj_000001.png")


def test_a_texcoord_list_of_the_wrong_length_is_refused(tmp_path):
    path = str(tmp_path / "m.ply")
    with open(path, "w") as out:
        out.write("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                  "element face 1\nproperty list uchar int vertex_indices\nproperty list uchar float texcoord\nend_header\n"
                  "0 0 0\n1 0 0\n0 1 0\n3 0 1 2 4 0 0 1 1\n")
    with pytest.raises(ValueError, match="texcoord list of 4 values on a face of 3 vertices"):
        metrics.load_ply_textured_mesh(path)


def test_load_texture_reads_grey_rgb_and_rgba_with_row_0_on_top(tmp_path):
    from PIL import Image
    rgb = tc.random_texture(5, 3)
    synth.write_png(str(tmp_path / "rgb.png"), rgb)
    assert np.array_equal(metrics.load_texture(str(tmp_path / "rgb.png")), rgb)
    grey = np.ascontiguousarray(rgb[:, :, 0])
    synth.write_png(str(tmp_path / "grey.png"), grey)
    assert np.array_equal(metrics.load_texture(str(tmp_path / "grey.png")), np.repeat(grey[:, :, None], 3, axis=2))
    rgba = np.concatenate([rgb, tc.random_texture(5, 3, 6)[:, :, :1]], axis=2)
    Image.fromarray(rgba, "RGBA").save(str(tmp_path / "rgba.png"))
    got = metrics.load_texture(str(tmp_path / "rgba.png"))
    assert got.shape == (3, 5, 3) and got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, rgb)


# ----------------------------------------------------------------------------------------------------------- 2. pyramid
@pytest.mark.parametrize("Wt,Ht", tc.TEXTURE_SIZES)
def test_pyramid_equals_the_box_filter(Wt, Ht):
    tex = tc.random_texture(Wt, Ht)
    mips = metrics.texture_mips(tex)
    want = tc.mips_np(tex)
    assert mips.levels == len(want) == metrics.texture_levels(Wt, Ht) and (mips.Wt, mips.Ht) == (Wt, Ht)
    assert mips.data.dtype == np.uint32 and len(mips.data) == sum(a.shape[0] * a.shape[1] for a in want)
    assert len(mips.data) * 4 == _lib.lib().bp_texture_mips_bytes(Wt, Ht, mips.levels)
    for l, a in enumerate(want):
        assert np.array_equal(mips.level(l), a), l
    assert want[-1].shape == (1, 1, 3) and not (mips.data >> 24).any()


def test_pyramid_sizes_and_the_clamped_partner():
    assert metrics.texture_mips(tc.random_texture(1, 1)).levels == 1
    assert [metrics.texture_levels(w, h) for w, h in tc.TEXTURE_SIZES] == [1, 4, 4, 4, 7]
    # 5 x 3: the last column of level 1 is the mean of column 4 with itself, the last row that of row 2 with itself
    tex = tc.random_texture(5, 3).astype(np.int64)
    l1 = metrics.texture_mips(tex.astype(np.uint8)).level(1)
    assert l1.shape == (2, 3, 3)
    assert np.array_equal(l1[0, 2], (2 * tex[0, 4] + 2 * tex[1, 4] + 2) >> 2)
    assert np.array_equal(l1[1, 0], (2 * tex[2, 0] + 2 * tex[2, 1] + 2) >> 2)
    assert np.array_equal(l1[1, 2], tex[2, 4])


# ---------------------------------------------------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("size", tc.SIZES)
@pytest.mark.parametrize("Wt,Ht", tc.TEXTURE_SIZES)
def test_identity_one_texel_per_pixel(size, Wt, Ht):
    """Texel centres on pixel centres: the covered window holds the texture's bytes, the top row on top.  The texture's
    values span 64 levels: a coordinate a rounding error below a texel centre moves 1/256 of the weight per axis to the
    neighbour, which changes no byte while neighbours differ by less than 64."""
    color, depth, skipped = tc.host("identity-%dx%d" % (Wt, Ht), size)
    tex = tc.random_texture(Wt, Ht, lo=96, hi=160)
    assert not skipped.any() and int((depth[0] > 0).sum()) == Wt * Ht
    assert (depth[0, 7:7 + Ht, 11:11 + Wt] > 0).all()
    assert np.array_equal(color[0, 7:7 + Ht, 11:11 + Wt], tex)
    if Ht > 1:
        assert not np.array_equal(color[0, 7:7 + Ht, 11:11 + Wt], tex[::-1])


# -------------------------------------------------------------------------------------------------------------- 4. flat
@pytest.mark.parametrize("size", tc.SIZES)
@pytest.mark.parametrize("mip", [True, False])
@pytest.mark.parametrize("Wt,Ht", [(8, 8), (1, 1)])
def test_flat_texture_equals_the_vertex_colour_path(size, Wt, Ht, mip):
    """One colour everywhere: colour, depth and skipped are render_color's with that colour on every vertex.  (Its
    channels are even: the vertex path mixes c with weights that sum to 1 within a rounding error, which could only
    matter where light_w c + 0.5 is an integer, and with light_w = 1/2 that takes an odd c.)"""
    got = tc.host("flat-%dx%d-%s" % (Wt, Ht, "mip" if mip else "base"), size)
    v, f = rc.torus()
    want = metrics.render_color(rc.poses_for("torus", size=size), v, f, np.tile(np.array(tc.FLAT, np.uint8), (len(v), 1)),
                                rc.camera(size), size, None, light=tc.LIGHT)
    assert (want[1] > 0).sum() > 1000
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------------ 5. minification
@pytest.mark.parametrize("size", tc.SIZES)
def test_minification_reads_a_coarser_level(size):
    """A one-texel checkerboard seen at three texels a pixel: every level from 1 on is the uniform grey 128, and that is
    what every pixel of the quad shows; without mip-mapping the same view aliases."""
    v, f, uv = tc.far_quad(size)
    _, rho2 = tc.render_np(tc.EYE, v, f, uv, tc.checkerboard(), rc.camera(size), size, ambient=1.0, want_rho=True)
    inside = np.isfinite(rho2)
    rho = np.sqrt(rho2[inside])
    assert inside.sum() >= 200 and rho.min() >= 2.5 and rho.max() <= 3.5
    for threshold in (2.0, 4.0):
        assert (np.abs(rho - threshold) > 0.1 * threshold).all()
    color, depth, _ = tc.host("minify-mip", size)
    assert np.array_equal(depth[0] > 0, inside)
    assert (color[0][inside] == 128).all() and not color[0][~inside].any()
    base = tc.host("minify-base", size)[0]
    assert len(np.unique(base[0][inside])) > 1 and (np.abs(base[0][inside].astype(int) - 128) > 100).mean() > 0.5


# ------------------------------------------------------------------------------------------------------- 6. perspective
@pytest.mark.parametrize("size", tc.SIZES)
@pytest.mark.parametrize("c", [0.0, 0.5])
def test_perspective_equals_the_restatement(size, c):
    v, f, uv, pose = tc.tilted_quad(size)
    want, rho2 = tc.render_np(pose, v, f, uv, tc.gradient_texture(), rc.camera(size), size, c, light=tc.LIGHT, want_rho=True)
    color, depth, skipped = tc.host("perspective-%.1f" % c, size)
    assert not skipped.any() and (depth[0] > 0).sum() > 1000
    levels = tc.level_np(rho2[np.isfinite(rho2)], rho2[np.isfinite(rho2)], 7)
    assert len(np.unique(levels)) >= 2                      # the tilt spreads the quad over more than one level
    assert np.array_equal(color[0], want)


# -------------------------------------------------------------------------------------------------------------- 7. wrap
@pytest.mark.parametrize("size", tc.SIZES)
def test_wrap_repeat_and_wild_coordinates(size):
    plain, shifted, bad = (tc.host("wrap-" + k, size) for k in ("plain", "shifted", "bad"))
    assert (plain[1] > 0).sum() > 1000
    for a, b in zip(plain, shifted):
        assert np.array_equal(a, b)
    v, f, uv, pose = tc.tilted_quad(size, angle=40.0)
    K = rc.camera(size)
    tex = tc.random_texture(5, 3)
    assert np.array_equal(plain[0][0], tc.render_np(pose, v, f, uv, tex, K, size, light=tc.LIGHT))
    # NaN, +-inf and 1e300 on face 1: a defined colour, the restatement's; face 0 keeps its bytes, depth is untouched
    assert np.array_equal(bad[0][0], tc.render_np(pose, v, f, tc.bad_uv(uv), tex, K, size, light=tc.LIGHT))
    face, _ = tc.winners(pose, v, f, K, size, 0.0)
    assert (face == 0).sum() > 300 and (face == 1).sum() > 300
    assert np.array_equal(bad[0][0][face == 0], plain[0][0][face == 0])
    assert np.array_equal(bad[1], plain[1]) and np.array_equal(bad[2], plain[2])


# ------------------------------------------------------------------------------------------------------------- 8. into=
@pytest.mark.parametrize("size", tc.SIZES)
def test_accumulation_across_the_two_kinds_of_call(size):
    """Textured over vertex-coloured and the reverse give the same images: a pixel belongs to the nearer mesh whichever
    was drawn first, and its bytes are those of that mesh drawn alone."""
    a = tc.host("into-textured-first", size)
    b = tc.host("into-textured-last", size)
    sphere_alone, box_alone = a[:3], b[:3]
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    sphere_wins = (sphere_alone[1] > 0) & ((box_alone[1] == 0) | (sphere_alone[1] < box_alone[1]))
    box_wins = (box_alone[1] > 0) & ((sphere_alone[1] == 0) | (box_alone[1] < sphere_alone[1]))
    assert ((box_alone[1] > 0) & sphere_wins).sum() > 200 and ((sphere_alone[1] > 0) & box_wins).sum() > 200
    assert np.array_equal(a[3][sphere_wins], sphere_alone[0][sphere_wins])
    assert np.array_equal(a[3][box_wins], box_alone[0][box_wins])


@pytest.mark.parametrize("size", tc.SIZES)
def test_the_later_call_wins_an_exact_tie(size):
    last_tex, depth, _ = tc.host("tie-textured-last", size)
    last_col, depth2, _ = tc.host("tie-textured-first", size)
    on = depth[0] > 0
    assert on.sum() > 100 and np.array_equal(depth, depth2)
    assert (last_tex[0][on] == [0, 0, 254]).all() and (last_col[0][on] == [254, 0, 0]).all()


# --------------------------------------------------------------------------------------------------------- 9. arguments
def _host_call(uv, mips, Wt, Ht, levels, F=2, colors=None):
    size = (16, 16)
    v, f, _ = tc.window_quad(2, 2, 4, 4, size)
    poses = np.ascontiguousarray(tc.EYE.reshape(1, 12))
    K = np.ascontiguousarray(rc.camera(size).reshape(9))
    light = np.zeros(3)
    color, depth, skipped = np.zeros((1, 16, 16, 3), np.uint8), np.zeros((1, 16, 16), np.float32), np.zeros(1, np.int32)
    rc_ = _lib.lib().bp_render_color_textured_host(_lib.ptr(poses), 1, _lib.ptr(v), 4, _lib.ptr(f), F, _lib.ptr(colors),
                                                   _lib.ptr(uv), _lib.ptr(mips), Wt, Ht, levels, None, 1, _lib.ptr(K), 16, 16,
                                                   0.0, 0.01, 0.5, _lib.ptr(light), 0, _lib.ptr(color), _lib.ptr(depth),
                                                   _lib.ptr(skipped))
    return rc_, _lib.lib().bp_last_error().decode(), color


def test_arguments_are_refused_by_name():
    size = (16, 16)
    v, f, uv = tc.window_quad(2, 2, 4, 4, size)
    tex = tc.random_texture(4, 4)
    K = rc.camera(size)
    for bad in (uv[:1], uv[:, :2], uv.reshape(2, 6)):
        with pytest.raises(ValueError, match=r"uv must have the shape \[F, 3, 2\]"):
            metrics.render_color(tc.EYE[None], v, f, None, K, size, uv=bad, texture=tex)
    with pytest.raises(ValueError, match="a texture needs uv"):
        metrics.render_color(tc.EYE[None], v, f, None, K, size, texture=tex)
    with pytest.raises(ValueError, match="uv without a texture"):
        metrics.render_color(tc.EYE[None], v, f, np.zeros((4, 3), np.uint8), K, size, uv=uv)
    with pytest.raises(ValueError, match="must not exceed 8192 x 8192"):
        metrics.texture_mips(np.zeros((1, 8193, 3), np.uint8))
    with pytest.raises(ValueError, match=r"uint8 array \[Ht, Wt, 3\]"):
        metrics.texture_mips(np.zeros((4, 4), np.uint8))
    # the library's own checks, before anything is touched
    mips = metrics.texture_mips(tex)
    rc_, text, color = _host_call(uv, mips.data, 4, 4, 3)
    assert rc_ == 0 and color.any()
    rc_, text, color = _host_call(uv, mips.data, 4, 4, 4)            # a 4 x 4 image has three levels
    assert rc_ == -1 and text.startswith("levels must lie in 1 ..") and not color.any()
    rc_, text, _ = _host_call(uv, mips.data, 4, 4, 0)
    assert rc_ == -1 and text.startswith("levels must lie in 1 ..")
    rc_, text, color = _host_call(uv, None, 4, 4, 3)
    assert rc_ == -1 and text.startswith("null argument: uv needs the pyramid") and not color.any()
    rc_, text, _ = _host_call(None, mips.data, 4, 4, 3)              # no uv: the vertex-colour call, which needs colours
    assert rc_ == -1 and text.startswith("null argument: uv needs the pyramid, no uv needs colors")
    rc_, text, _ = _host_call(uv, mips.data, 8193, 4, 1)
    assert rc_ == -1 and text.startswith("a texture must not exceed 8192 x 8192")
    rc_, text, _ = _host_call(uv, mips.data, 4, 0, 1)
    assert rc_ == -1 and text.startswith("Wt and Ht must be positive")
    rc_, text, _ = _host_call(uv, mips.data, 4, 4, 3, F=0)
    assert rc_ == -1 and "must be positive" in text
    lib = _lib.lib()
    assert lib.bp_texture_mips_bytes(8193, 1, 1) == 0 and lib.bp_texture_mips_bytes(4, 4, 4) == 0
    assert lib.bp_texture_mips_bytes(4, 4, 3) == 4 * (16 + 4 + 1) and lib.bp_texture_mips_bytes(8192, 8192, 14) > 0
    out = np.zeros(21, np.uint32)
    assert lib.bp_texture_mips_host(_lib.ptr(tex), 8193, 4, 1, _lib.ptr(out)) == -1
    assert lib.bp_last_error().decode().startswith("a texture must not exceed 8192 x 8192")
    assert lib.bp_texture_mips_host(None, 4, 4, 3, _lib.ptr(out)) == -1 and lib.bp_last_error().startswith(b"null argument")
    assert not out.any()
    # no uv and colours: the entry is bp_render_color_host
    col = tc.random_texture(4, 1)[0]
    rc_, _, color = _host_call(None, None, 0, 0, 0, colors=np.ascontiguousarray(col))
    assert rc_ == 0 and np.array_equal(color, metrics.render_color(tc.EYE[None], v, f, col, K, size)[0])


def test_a_pyramid_is_built_for_the_place_it_is_used():
    size = (16, 16)
    v, f, uv = tc.window_quad(2, 2, 4, 4, size)
    mips = metrics.texture_mips(tc.random_texture(4, 4))
    with pytest.raises(ValueError, match="the pyramid was built for the host"):
        metrics.render_color(tc.EYE[None], v, f, None, rc.camera(size), size, "cuda:0", uv=uv, texture=mips)
    a = metrics.render_color(tc.EYE[None], v, f, None, rc.camera(size), size, uv=uv, texture=mips)
    b = metrics.render_color(tc.EYE[None], v, f, None, rc.camera(size), size, uv=uv, texture=tc.random_texture(4, 4))
    assert np.array_equal(a[0], b[0]) and a[0].any()


# ------------------------------------------------------------------------------------------------------ 10. synthesiser
SAME_KEYS = ["depth", "obj_ids", "poses", "t_mm", "present", "box_full", "box_visible", "visib_fract", "redraws", "params"]


@pytest.mark.parametrize("kind", ["scenes", "multi"])
def test_synthesiser_takes_a_textured_mesh(kind):
    """Only the frames change with a texture, and there only where the textured object shows; chunks concatenate."""
    plain, tex = tc.host_synth(kind, False), tc.host_synth(kind, True)
    assert set(plain) == set(tex)
    for key in plain:
        if key != "frames":
            assert np.array_equal(plain[key], tex[key]), key
    assert set(SAME_KEYS) <= set(plain) and tex["frames"].shape == (3,) + tc.SYNTH_SIZE + (3,)
    changed = (plain["frames"] != tex["frames"]).any(axis=-1)
    assert changed.reshape(3, -1).sum(axis=1).min() > 50
    if kind == "multi":
        assert tex["present"][:, 0].all()
    run = tc.synth_scenes if kind == "scenes" else tc.synth_multi
    parts = [run(True, 2), run(True, 1, first_scene=2)]
    for key in tex:
        if key != "obj_ids":
            assert np.array_equal(np.concatenate([p[key] for p in parts]), tex[key]), key


def test_synthesiser_swaps_the_texture_to_bgr_once():
    """The frames are BGR: a texture that is red in RGB comes out in channel 2, as red vertex colours do."""
    from betapose_amd import synth as S
    sv, sf = rc.icosphere()
    red = np.zeros((2, 2, 3), np.uint8)
    red[:, :, 0] = 254
    K = rc.camera(tc.SYNTH_SIZE)
    kw = dict(camera=dict(feather=0, blur=0, gain=256, offset=0, sigma=0), sensor=dict(noise_k=0, hole_p=0), ambient=1.0)
    a = S.synthesize_scenes((sv * 0.05, sf, None, tc.corner_uv(len(sf)), red), [], K, tc.SYNTH_SIZE, 1, 1, **kw)
    b = S.synthesize_scenes((sv * 0.05, sf, np.tile(red[0, 0], (len(sv), 1))), [], K, tc.SYNTH_SIZE, 1, 1, **kw)
    assert np.array_equal(a["frames"], b["frames"])
    on = a["depth"][0] > 0
    inner = on & np.roll(on, 1, 0) & np.roll(on, -1, 0) & np.roll(on, 1, 1) & np.roll(on, -1, 1)
    assert inner.sum() > 100 and (a["frames"][0][inner] == [0, 0, 254]).all()


# --------------------------------------------------------------------------------------------------------- command line
def _write_textured_ply(path, texture_file):
    """The icosphere in millimetres with vertex colours, per-vertex texture coordinates and (or not) a TextureFile."""
    import synth_common as sc
    v, f = rc.icosphere()
    col = sc.vertex_colors(len(v), 11)
    uv = np.random.default_rng(2).integers(0, 9, size=(len(v), 2)) / 8.0
    with open(path, "w") as out:
        out.write("ply\nformat ascii 1.0\n" + ("comment TextureFile %s\n" % texture_file if texture_file else "") +
                  "element vertex %d\nproperty double x\nproperty double y\nproperty double z\nproperty uchar red\n"
                  "property uchar green\nproperty uchar blue\nproperty float texture_u\nproperty float texture_v\n"
                  "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
        for p, c, t in zip(v * 50.0, col, uv):
            out.write(" ".join(repr(float(x)) for x in p) + " %d %d %d %r %r\n" % (c[0], c[1], c[2], float(t[0]), float(t[1])))
        for a, b, c in f:
            out.write("3 %d %d %d\n" % (a, b, c))


def test_synthesize_py_uses_a_plys_texture(tmp_path):
    """--model with a TextureFile writes textured frames; --no_texture writes the files of a PLY that names none; every
    file but the RGB images is the same in all three; a named file that is missing is an error that names it."""
    import importlib
    import synth_multi_common as mc
    synthesize = importlib.import_module("synthesize")
    synth.write_png(str(tmp_path / "skin.png"), tc.gradient_texture())
    _write_textured_ply(str(tmp_path / "textured.ply"), "skin.png")
    _write_textured_ply(str(tmp_path / "plain.ply"), None)
    args = ["--frames", "2", "--size", "48x64", "--camera", "60,60,31.5,23.5", "--seed", "3"]
    runs = {"tex": ["--model", str(tmp_path / "textured.ply")], "off": ["--model", str(tmp_path / "textured.ply"), "--no_texture"],
            "plain": ["--model", str(tmp_path / "plain.ply")]}
    for name, extra in runs.items():
        assert synthesize.main(extra + ["--out", str(tmp_path / name)] + args) == 0
    assert mc.tree_digest(str(tmp_path / "off")) == mc.tree_digest(str(tmp_path / "plain"))
    assert mc.tree_digest(str(tmp_path / "tex")) != mc.tree_digest(str(tmp_path / "plain"))
    from PIL import Image
    for nr in range(2):
        rgb = [np.asarray(Image.open(str(tmp_path / name / "test" / "01" / "rgb" / ("%04d.png" % nr)))) for name in ("tex", "plain")]
        assert (rgb[0] != rgb[1]).any(axis=-1).sum() > 50
        depth = [np.asarray(Image.open(str(tmp_path / name / "test" / "01" / "depth" / ("%04d.png" % nr)))) for name in ("tex", "plain")]
        assert np.array_equal(depth[0], depth[1])
    for name in ("gt.yml", "info.yml"):
        assert (tmp_path / "tex" / "test" / "01" / name).read_bytes() == (tmp_path / "plain" / "test" / "01" / name).read_bytes()
    _write_textured_ply(str(tmp_path / "lost.ply"), "nowhere.png")
    with pytest.raises(SystemExit, match="nowhere.png, which does not exist"):
        synthesize.main(["--model", str(tmp_path / "lost.ply"), "--out", str(tmp_path / "lost")] + args)
    assert synthesize.main(["--model", str(tmp_path / "lost.ply"), "--no_texture", "--out", str(tmp_path / "lost")] + args) == 0
