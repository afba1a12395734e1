"""The training-scene synthesiser's kernels (csrc/synth.hip) against their host twins, byte for byte: every case of
synth_common at 48 x 64 and 75 x 113 (every compose tile partial), compose once at 129 x 67, one 480 x 640 image per
kernel (the real row length, 16-byte stores, several thousand tiles), outputs pre-filled with a marker byte, a second
stream, the chunking identity, and synthesize_scenes as a whole.  The host twins themselves are checked against the
definitions in test_synth_host.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raster_common as rc  # noqa: E402
import synth_common as sc  # noqa: E402
from betapose_amd import _lib, synth  # noqa: E402

DEV = "cuda:0"


@pytest.mark.parametrize("size", sc.SIZES)
def test_backgrounds_and_windows_equal_the_host(size):
    assert np.array_equal(synth.procedural_background(3, size, sc.SEED, 7, DEV), sc.host_background(size))
    assert np.array_equal(synth.background_windows(sc.bank(), sc.WINDOWS, size, DEV), sc.host_windows(size))


@pytest.mark.parametrize("r,feather", sc.COMPOSE_CASES)
@pytest.mark.parametrize("size", sc.SIZES)
def test_compose_equals_the_host(size, r, feather):
    color, depth = sc.scene_stack(size)
    got = synth.compose(sc.backgrounds(size), color, depth, sc.compose_table(r, feather), sc.SEED, 7, DEV)
    assert np.array_equal(got, sc.host_compose(size, r, feather))


def test_compose_tall_image_equals_the_host():
    color, depth = sc.scene_stack(sc.TALL)
    table = sc.compose_table(2, 1)
    want = synth.compose(sc.backgrounds(sc.TALL), color, depth, table, sc.SEED, 7)
    assert np.array_equal(synth.compose(sc.backgrounds(sc.TALL), color, depth, table, sc.SEED, 7, DEV), want)


@pytest.mark.parametrize("size", sc.SIZES)
def test_sensor_depth_equals_the_host(size):
    got = synth.sensor_depth(sc.scene_stack(size)[1], sc.DEPTH_SCALE, sc.SENSOR_ROWS, sc.SEED, 7, DEV)
    assert np.array_equal(got, sc.host_sensor(size))


def test_full_frame_with_marked_outputs():
    """One 480 x 640 image per kernel, straight through the C entry points into outputs pre-filled with a marker byte:
    equal to the host twin means every byte was written.  640 is a multiple of 16, so these are the 16-byte store
    paths of the background and compose kernels (7.5 x 10 tiles' worth of rows: the last tile row is half outside)."""
    import torch
    from betapose_amd import metrics
    size = (480, 640)
    H, W = size
    K = rc.camera(size)
    tv, tf = rc.torus()
    pose = rc.poses_for("torus", 1, size)
    color, depth, _ = metrics.render_color(pose, tv, tf, sc.vertex_colors(len(tv), 4), K, size)
    bg = sc.backgrounds(size, 1)
    table = np.array([[1, 2, 300, 250, 270, 5, -7, 11, 1500]], np.int32)
    rows = sc.SENSOR_ROWS[1:2]
    want_bg = synth.procedural_background(1, size, sc.SEED, 3)
    want_frame = synth.compose(bg, color, depth, table, sc.SEED, 3)
    want_depth = synth.sensor_depth(depth, sc.DEPTH_SCALE, rows, sc.SEED, 3)
    L, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
    for marker in (0xA5, 0x5A):
        d_out = torch.full((1, H, W, 3), marker, dtype=torch.uint8, device=DEV)
        _lib.check(L.bp_synth_background(1, H, W, sc.SEED, 3, _lib.ptr(d_out), s))
        assert np.array_equal(d_out.cpu().numpy(), want_bg)
        d_bg, d_color, d_depth = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (bg, color, depth))
        d_out = torch.full((1, H, W, 3), marker, dtype=torch.uint8, device=DEV)
        _lib.check(L.bp_synth_compose(_lib.ptr(d_bg), _lib.ptr(d_color), _lib.ptr(d_depth), 1, H, W, _lib.ptr(table), sc.SEED, 3,
                                      _lib.ptr(d_out), s))
        assert np.array_equal(d_out.cpu().numpy(), want_frame)
        d_u16 = torch.full((1, H, W), marker * 257 - 65536 if marker * 257 > 32767 else marker * 257, dtype=torch.int16, device=DEV)
        _lib.check(L.bp_synth_sensor_depth(_lib.ptr(d_depth), 1, H, W, sc.DEPTH_SCALE, _lib.ptr(rows), sc.SEED, 3, _lib.ptr(d_u16), s))
        assert np.array_equal(d_u16.cpu().numpy().view(np.uint16), want_depth)
    win = np.array([[1, 3, 2, 47, 31, 1]], np.int32)
    assert np.array_equal(synth.background_windows(sc.bank(), win, size, DEV), synth.background_windows(sc.bank(), win, size))


def test_unaligned_output_takes_the_byte_stores():
    """The same 16-column image written one byte into an allocation: the 16-byte paths must step aside."""
    import torch
    size = (32, 64)
    H, W = size
    color, depth = np.zeros((1, H, W, 3), np.uint8), np.zeros((1, H, W), np.float32)
    depth[0, 5:20, 10:50] = 1.0
    color[0, 5:20, 10:50] = (10, 200, 90)
    bg = sc.backgrounds(size, 1)
    table = sc.compose_table(1, 1, 1)
    L, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d_bg, d_color, d_depth = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (bg, color, depth))
    buf = torch.full((H * W * 3 + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(L.bp_synth_compose(_lib.ptr(d_bg), _lib.ptr(d_color), _lib.ptr(d_depth), 1, H, W, _lib.ptr(table), 9, 0,
                                  buf.data_ptr() + 1, s))
    got = buf.cpu().numpy()
    assert np.array_equal(got[1:-15].reshape(1, H, W, 3), synth.compose(bg, color, depth, table, 9, 0))
    assert got[0] == 0xA5 and (got[-15:] == 0xA5).all()
    buf.fill_(0xA5)
    _lib.check(L.bp_synth_background(1, H, W, 9, 0, buf.data_ptr() + 1, s))
    got = buf.cpu().numpy()
    assert np.array_equal(got[1:-15].reshape(1, H, W, 3), synth.procedural_background(1, size, 9, 0))
    assert got[0] == 0xA5 and (got[-15:] == 0xA5).all()


def test_second_stream_and_chunks():
    import torch
    size = sc.SIZES[1]
    color, depth = sc.scene_stack(size)
    bg, table = sc.backgrounds(size), sc.compose_table(2, 1)
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        assert np.array_equal(synth.compose(bg, color, depth, table, sc.SEED, 7, DEV), sc.host_compose(size, 2, 1))
        assert np.array_equal(synth.sensor_depth(depth, sc.DEPTH_SCALE, sc.SENSOR_ROWS, sc.SEED, 7, DEV), sc.host_sensor(size))
        assert np.array_equal(synth.procedural_background(3, size, sc.SEED, 7, DEV), sc.host_background(size))
    for i in range(3):                           # scenes 7, 8, 9 one at a time equal the call that made all of them
        s = slice(i, i + 1)
        assert np.array_equal(synth.compose(bg[s], color[s], depth[s], table[s], sc.SEED, 7 + i, DEV), sc.host_compose(size, 2, 1)[s])
        assert np.array_equal(synth.sensor_depth(depth[s], sc.DEPTH_SCALE, sc.SENSOR_ROWS[s], sc.SEED, 7 + i, DEV), sc.host_sensor(size)[s])
        assert np.array_equal(synth.procedural_background(1, size, sc.SEED, 7 + i, DEV), sc.host_background(size)[s])


def test_more_images_than_one_launch_holds():
    """66 images: the tables travel as kernel arguments, 64 images per launch, so the last two are a launch of their own."""
    size = (16, 24)
    rng = np.random.default_rng(3)
    n = 66
    bg = rng.integers(0, 256, (n,) + size + (3,)).astype(np.uint8)
    color = rng.integers(0, 256, (n,) + size + (3,)).astype(np.uint8)
    depth = (rng.uniform(0, 1, (n,) + size) > 0.5).astype(np.float32) * rng.uniform(0.5, 2.0, (n,) + size).astype(np.float32)
    table = np.concatenate([sc.compose_table(r, f) for r, f in sc.COMPOSE_CASES] * 3)[:n]
    rows = np.tile(sc.SENSOR_ROWS, (14, 1))[:n]
    assert np.array_equal(synth.compose(bg, color, depth, table, 1, 0, DEV), synth.compose(bg, color, depth, table, 1, 0))
    assert np.array_equal(synth.sensor_depth(depth, 0.001, rows, 1, 0, DEV), synth.sensor_depth(depth, 0.001, rows, 1, 0))
    assert np.array_equal(synth.procedural_background(n, size, 1, 0, DEV), synth.procedural_background(n, size, 1, 0))


def test_synthesize_scenes_on_the_device_equals_the_host():
    host, dev = sc.synthesize(4, sensor={}), sc.synthesize(4, DEV, sensor={})
    assert set(host) == set(dev)
    for key in host:
        assert np.array_equal(host[key], dev[key]), key
