"""bp_render_color, bp_draw_boxes and bp_overlay (csrc/raster_color.hip) against their host twins, byte for byte: the
colour bytes, the depth bits and the skipped counts of every case of test_render_color_host.py (render_color_common.CASES),
bad face indices, pre-filled outputs, a second stream and the Renderer on a device.  A few launches each.

Image sizes (raster_common.SIZES): 48 x 64 wherever no size is named (W = the wave width); 75 x 113 for every case that
takes a size (W an odd prime above the wave width: the per-pixel kernels' ``i / W`` is a division, a lane changes its column
with every pixel, and the cooperative-wave visibility path walks boxes whose width is no multiple of 64); 129 x 67 once
(H > W, W three past a wave)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raster_common as rc  # noqa: E402
import render_color_common as cc  # noqa: E402

H, W, K = rc.H, rc.W, rc.K
FILL = 7


def assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_parity_with_the_host_twin(name):
    want = cc.host(name)
    assert_same(cc.CASES[name]("cuda"), want)
    if name == "edge-box_closeup":                  # 12 triangles over the whole frame: the cooperative-wave path
        assert (want[1] > 0).mean() > 0.9
    if name == "edge-behind_near":
        assert want[2][0] > 0


@pytest.mark.parametrize("name", cc.SIZE_FREE)
def test_parity_with_the_host_twin_at_75x113(name):
    """Every case that takes an image size on a 113 x 75 image: rows of an odd prime length above the wave width, where
    a lane of the per-pixel kernels changes its column with every pixel (raster_common.SIZES)."""
    size = (75, 113)
    want = cc.host(name, size)
    assert want[0].shape[1:3] == size
    assert_same(cc.CASES[name]("cuda", size), want)
    if name == "edge-box_closeup":
        assert (want[1] > 0).mean() > 0.9
    if name == "edge-behind_near":
        assert want[2][0] > 0


def test_parity_with_the_host_twin_at_129x67():
    """An image higher than wide, W three past a wave: the torus' four poses, shaded."""
    size = (129, 67)
    want = cc.host("mesh-torus-0.0", size)
    assert want[0].shape == (4, 129, 67, 3) and (want[1] > 0).any(axis=(1, 2)).all()
    assert_same(cc.CASES["mesh-torus-0.0"]("cuda", size), want)


def device_render_color(poses, v, f, colors, index=None, images=None, accumulate=0, stream=None, near=0.01):
    """The raw call with every output pre-filled with FILL."""
    import torch
    from betapose_amd import _lib
    poses = np.ascontiguousarray(np.asarray(poses, np.float64)[:, :3, :4]).reshape(-1, 12)
    images = len(poses) if images is None else images
    d_model = torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda()
    d_faces = torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()
    d_colors = torch.from_numpy(np.ascontiguousarray(colors, np.uint8)).cuda()
    d_poses = torch.from_numpy(poses).cuda()
    d_color = torch.full((images, H, W, 3), FILL, dtype=torch.uint8, device="cuda")
    d_depth = torch.full((images, H, W), float(FILL), dtype=torch.float32, device="cuda")
    d_skipped = torch.full((len(poses),), FILL, dtype=torch.int32, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    index = None if index is None else np.ascontiguousarray(index, np.int32)
    _lib.check(_lib.lib().bp_render_color(_lib.ptr(d_model), len(v), _lib.ptr(d_faces), len(f), _lib.ptr(d_colors),
                                          _lib.ptr(d_poses), len(poses), _lib.ptr(index), images,
                                          _lib.ptr(np.ascontiguousarray(K).reshape(9)), H, W, 0.0, near, 0.5,
                                          _lib.ptr(np.zeros(3)), accumulate, _lib.ptr(d_color), _lib.ptr(d_depth),
                                          _lib.ptr(d_skipped), s.cuda_stream))
    return d_color.cpu().numpy(), d_depth.cpu().numpy(), d_skipped.cpu().numpy()


def test_bad_face_index_is_skipped_and_counted():
    """The device call cannot refuse an index it has not read: the kernel skips the two triangles and counts them, and
    the image is the host's of the mesh without them."""
    from betapose_amd import metrics
    v, f = rc.box()
    col = cc.colors_for(len(v))
    pose = np.eye(4)[None, :3].copy()
    pose[0, 2, 3] = 3.0
    bad = f.copy()
    bad[3, 1], bad[7, 0] = len(v), -1
    color, depth, skipped = device_render_color(pose, v, bad, col)
    assert skipped[0] == 2
    keep = np.ones(len(f), bool)
    keep[[3, 7]] = False
    want = metrics.render_color(pose, v, f[keep], col, K, (H, W))
    assert_same((color, depth), want[:2])


def test_prefilled_outputs_five_poses_repeats_and_second_stream():
    """Without accumulate the sentinel disappears from every byte; P = 5 poses over 3 images, twice on the current stream
    and once on another: all byte-identical to the host."""
    import torch
    from betapose_amd import metrics
    v, f = rc.torus()
    col = cc.colors_for(len(v))
    poses = np.concatenate([rc.poses_for("torus"), rc.poses_for("torus", 6)[5:]])
    index = [0, 0, 1, 2, 2]
    want = metrics.render_color(poses, v, f, col, K, (H, W), image_index=index, images=3)
    first = device_render_color(poses, v, f, col, index, 3)
    assert_same(first, want)
    assert (first[1] == 0).any() and not (first[1] == FILL).any()
    assert_same(device_render_color(poses, v, f, col, index, 3), first)
    assert_same(device_render_color(poses, v, f, col, index, 3, stream=torch.cuda.Stream()), first)
    torch.cuda.synchronize()


def test_renderer_on_the_device_equals_the_host():
    from betapose_amd import metrics
    from betapose_amd.renderer import Renderer, draw_poses

    class Model:
        pass
    (sv, sf, sc, ps), (bv, bf, bc, pb), _ = cc.two_mesh_scene()
    out = []
    for device in (None, "cuda"):
        ren = Renderer((W, H), K, device)
        models = []
        for v, f, c in ((sv, sf, sc), (bv, bf, bc)):
            m = Model()
            m.vertices, m.indices, m.colors, m.bb = v, f, c / 255.0, metrics.box_corners(v)
            models.append(m)
        ren.draw_model(models[0], ps)
        ren.draw_model(models[1], pb)
        ren.draw_boundingbox(models[1], pb)
        rgb, dep = ren.finish()
        frame = np.random.default_rng(5).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        out.append((rgb, dep, ren.drawn, draw_poses(frame, np.stack([ps, pb]), models[1], K, device=device)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert out[0][2].any()


def test_device_entry_points_refuse_bad_arguments():
    import torch
    from betapose_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    v, f = rc.box()
    d = {k: torch.zeros(n, dtype=t, device="cuda") for k, n, t in
         [("model", 24, torch.float64), ("faces", 36, torch.int32), ("colors", 24, torch.uint8), ("poses", 24, torch.float64),
          ("color", 2 * H * W * 3, torch.uint8), ("depth", 2 * H * W, torch.float32), ("skipped", 2, torch.int32)]}
    d["faces"].copy_(torch.from_numpy(f.reshape(-1)))
    Kf, light, index = np.ascontiguousarray(K).reshape(9), np.zeros(3), np.array([0, 1], np.int32)
    good = [p(d["model"]), 8, p(d["faces"]), 12, p(d["colors"]), p(d["poses"]), 2, p(index), 2, p(Kf), H, W, 0.0, 0.01, 0.5,
            p(light), 0, p(d["color"]), p(d["depth"]), p(d["skipped"]), None]
    assert L.bp_render_color(*good) == 0
    for ch in [(0, None), (2, None), (4, None), (5, None), (9, None), (15, None), (17, None), (18, None), (19, None), (1, 0), (3, 0),
               (6, 0), (8, 0), (10, 0), (11, -1), (13, 0.0), (7, p(np.array([1, 0], np.int32))), (7, p(np.array([0, 2], np.int32))),
               (7, None, 8, 3), (10, 4097, 11, 4096), (3, 1 << 16, 6, 1 << 16, 7, None, 8, 1 << 16)]:
        args = list(good)
        for i in range(0, len(ch), 2):
            args[ch[i]] = ch[i + 1]
        assert L.bp_render_color(*args) < 0 and L.bp_last_error(), ch
    corners = torch.zeros(24, dtype=torch.float64, device="cuda")
    good = [p(d["poses"]), 2, p(corners), p(d["colors"]), p(index), 2, p(Kf), H, W, 0.0, 0.01, p(d["color"]), None]
    assert L.bp_draw_boxes(*good) == 0
    for ch in [(0, None), (2, None), (3, None), (6, None), (11, None), (1, 0), (5, 0), (7, 0), (10, 0.0),
               (4, p(np.array([1, 0], np.int32))), (4, None, 5, 1)]:
        args = list(good)
        for i in range(0, len(ch), 2):
            args[ch[i]] = ch[i + 1]
        assert L.bp_draw_boxes(*args) < 0 and L.bp_last_error(), ch
    render = torch.zeros_like(d["color"])
    good = [p(d["color"]), p(render), p(d["depth"]), 2, H, W, 128, p(d["color"]), None]        # (out may be frames)
    assert L.bp_overlay(*good) == 0
    for ch in [(0, None), (1, None), (2, None), (7, None), (3, 0), (6, 257), (6, -1)]:
        args = list(good)
        args[ch[0]] = ch[1]
        assert L.bp_overlay(*args) < 0 and L.bp_last_error(), ch
    torch.cuda.synchronize()
