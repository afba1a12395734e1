"""The instance kernels (csrc/synth_inst.hip) against their host twin, byte for byte: every stack of synth_multi_common
at 48 x 64 (16-byte loads, 4-byte id stores) and 75 x 113 (H W no multiple of 4: the scalar path) with 1, 3 and 32
objects, the rendered stacks with their ties, one 480 x 640 image into outputs pre-filled with a marker byte, outputs
and inputs moved off their alignment, a second stream, 70 tiny images, and synthesize_multi as a whole.  The host twin
itself is checked against the definitions in test_synth_multi_host.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raster_common as rc  # noqa: E402
import synth_multi_common as mc  # noqa: E402
from betapose_amd import _lib, synth  # noqa: E402

DEV = "cuda:0"


def _same(got, want):
    for g, w, name in zip(got, want, ("ids", "depth", "stats")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name


@pytest.mark.parametrize("J", mc.OBJECTS)
@pytest.mark.parametrize("size", mc.SIZES)
def test_instance_masks_equal_the_host(size, J):
    _same(synth.instance_masks(*mc.random_stack(size, J), device=DEV), mc.host_instances(size, J))


@pytest.mark.parametrize("size", mc.SIZES)
def test_rendered_stacks_and_ties_equal_the_host(size):
    alone, _, present = mc.rendered_stack(size)
    _same(synth.instance_masks(alone, present, DEV), synth.instance_masks(alone, present))
    pair = np.ascontiguousarray(alone[[0, 3]])
    got = synth.instance_masks(pair, None, DEV)
    _same(got, synth.instance_masks(pair))
    assert set(np.unique(got[0])) == {0, 2} and (got[2][:, 0, 1] == 0).all()             # the higher object owns every tie


def _call(alone, present, marker, stream=None, ids_shift=0, depth_shift=0, alone_shift=0):
    """bp_synth_instances through the C entry into outputs pre-filled with ``marker``, each tensor ``*_shift`` bytes into
    an allocation 16 bytes larger: (ids, depth, stats) and the three guard regions."""
    import torch
    J, I, H, W = alone.shape
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    d_alone = torch.full((alone.nbytes + 16,), marker, dtype=torch.uint8, device=DEV)
    d_alone[alone_shift:alone_shift + alone.nbytes] = torch.from_numpy(np.ascontiguousarray(alone).view(np.uint8).reshape(-1).copy()).to(DEV)
    d_present = torch.from_numpy(np.ascontiguousarray(present, dtype=np.uint8).copy()).to(DEV)
    d_ids = torch.full((I * H * W + 16,), marker, dtype=torch.uint8, device=DEV)
    d_depth = torch.full((I * H * W * 4 + 16,), marker, dtype=torch.uint8, device=DEV)
    d_stats = torch.full((I * J * 10 * 4,), marker, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().bp_synth_instances(d_alone.data_ptr() + alone_shift, J, I, H, W, _lib.ptr(d_present), d_ids.data_ptr() + ids_shift,
                                             d_depth.data_ptr() + depth_shift, _lib.ptr(d_stats), s))
    if stream is not None:
        stream.synchronize()
    ids, depth = d_ids.cpu().numpy(), d_depth.cpu().numpy()
    cut = lambda a, shift, n: (a[shift:shift + n], np.concatenate([a[:shift], a[shift + n:]]))
    (ids, g0), (depth, g1) = cut(ids, ids_shift, I * H * W), cut(depth, depth_shift, I * H * W * 4)
    assert (g0 == marker).all() and (g1 == marker).all()                                 # nothing outside the tensors
    return ids.reshape(I, H, W), depth.view(np.float32).reshape(I, H, W), d_stats.cpu().numpy().view(np.int32).reshape(I, J, 10)


@pytest.fixture(scope="module")
def full_frame():
    """One 480 x 640 scene of four objects that overlap round the middle of the image."""
    from betapose_amd import metrics
    size = (480, 640)
    K = rc.camera(size)
    objs = mc.render_objects()
    _, poses, _ = mc.rendered_stack((48, 64))
    alone = np.stack([metrics.render_depth(poses[:1, j], objs[j][0], objs[j][1], K, size)[0] for j in range(4)])
    present = np.ones((1, 4), np.uint8)
    return alone, present, synth.instance_masks(alone, present)


def test_full_frame_with_marked_outputs(full_frame):
    """Equal to the host twin from two different markers: every byte of ids, depth and stats was written."""
    alone, present, want = full_frame
    assert len(np.unique(want[0])) >= 3
    for marker in (0xA5, 0x5A):
        _same(_call(alone, present, marker), want)


def test_tensors_off_their_alignment_take_the_scalar_accesses():
    """W = 64: the stacks of the aligned path, with ids one byte, then depth and the lone renders one float, into their
    allocations; the guard bytes round them stay as they were (checked in _call)."""
    alone, present = mc.random_stack((48, 64), 3)
    want = mc.host_instances((48, 64), 3)
    _same(_call(alone, present, 0xA5, ids_shift=1), want)
    _same(_call(alone, present, 0xA5, depth_shift=4), want)
    _same(_call(alone, present, 0xA5, alone_shift=4), want)
    _same(_call(alone, present, 0xA5, ids_shift=3, depth_shift=12, alone_shift=8), want)


def test_second_stream():
    import torch
    alone, present = mc.random_stack((75, 113), 3)
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        _same(synth.instance_masks(alone, present, DEV), mc.host_instances((75, 113), 3))
    _same(_call(alone, present, 0x5A, stream=stream), mc.host_instances((75, 113), 3))


def test_seventy_tiny_images():
    alone, present = mc.random_stack((5, 7), 3, images=70, seed=1)
    want = synth.instance_masks(alone, present)
    _same(synth.instance_masks(alone, present, DEV), want)
    assert (want[2][:, :2, 0] > 0).all()


def test_a_scene_without_objects_is_empty():
    alone, _ = mc.random_stack((48, 64), 3)
    present = np.ones((mc.IMAGES, 3), np.uint8)
    present[0] = 0
    ids, depth, stats = _call(alone, present, 0xA5)
    assert not ids[0].any() and not depth[0].any() and (stats[0, :, 1] == 0).all() and (stats[0, :, 6:] == -1).all()
    assert (stats[0, :2, 0] > 0).all() and ids[1].any()
    _same((ids, depth, stats), synth.instance_masks(alone, present))


def test_entry_refuses_what_it_cannot_index():
    import torch
    lib = _lib.lib()
    d = torch.zeros(64, dtype=torch.float32, device=DEV)
    call = lambda J, I, H, W: lib.bp_synth_instances(_lib.ptr(d), J, I, H, W, _lib.ptr(d), _lib.ptr(d), _lib.ptr(d[32:]), _lib.ptr(d), None)
    for args, word in (((0, 1, 2, 2), "J must lie"), ((33, 1, 2, 2), "J must lie"), ((1, 1, 4097, 4096), "2^24")):
        assert call(*args) == -1 and word in lib.bp_last_error().decode()
    torch.cuda.synchronize()


def test_synthesize_multi_equals_the_host():
    got, want = mc.synthesize_multi(4, device=DEV), mc.host_multi()
    assert set(got) == set(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
