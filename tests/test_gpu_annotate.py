"""The key-point annotator's kernels (csrc/annotate.hip: bp_annotate_keypoints, bp_mask_boxes, bp_vertex_boxes,
bp_kpd_targets) against their host twins, bit for bit: uint64 / uint32 views of the floats, array_equal of the integers.
Images of 37 x 70 (W neither a multiple of 64 nor of 4) and 480 x 640, P = 5 poses with an empty render, an object cut by
the image border and one behind the camera, n = 500 vertices (and one count past a block's slice), Kp = 7, targets at
B = 3 with 80 x 64 and 13 x 10 maps.  Every output buffer is pre-filled with a sentinel; every function runs twice and
once on a second stream."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import annotate_common as ac  # noqa: E402

SIZES = [(37, 70), (480, 640)]
FILL = 113


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared scene is read-only)


def _runs(call):
    """call(stream) three times: twice on the current stream, once on a second one; the results must all be equal."""
    import torch
    first, again = call(None), call(None)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    other = call(side)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    return first


def _stream(s):
    import torch
    return (s if s is not None else torch.cuda.current_stream()).cuda_stream


def device_keypoints(sc, model_depth, scene, index, c=0.0, near=0.01, tol=0.015, delta=0.015):
    import torch
    from betapose_amd import _lib
    H, W = sc["size"]
    P, Kp = len(sc["poses"]), len(sc["kp"])
    d = [_dev(sc["poses"].reshape(P, 12)), _dev(sc["kp"]), _dev(model_depth), _dev(scene), _dev(index)]
    Kf = np.ascontiguousarray(sc["K"]).reshape(9)

    def call(s):
        xy = torch.full((P, Kp, 2), float(FILL), dtype=torch.float64, device="cuda")
        z = torch.full((P, Kp), float(FILL), dtype=torch.float64, device="cuda")
        fl = torch.full((P, Kp), FILL, dtype=torch.uint8, device="cuda")
        if s is not None:
            s.wait_stream(torch.cuda.current_stream())
        _lib.check(_lib.lib().bp_annotate_keypoints(_lib.ptr(d[0]), P, _lib.ptr(d[1]), Kp, _lib.ptr(Kf), H, W, c, near,
                                                    _lib.ptr(d[2]), _lib.ptr(d[3]), 0 if scene is None else len(scene),
                                                    _lib.ptr(d[4]), tol, delta, _lib.ptr(xy), _lib.ptr(z), _lib.ptr(fl), _stream(s)))
        if s is not None:
            s.synchronize()
        return xy.cpu().numpy(), z.cpu().numpy(), fl.cpu().numpy()
    return _runs(call)


@pytest.mark.parametrize("size", SIZES)
def test_keypoints_parity(size):
    from betapose_amd import annotate as A
    sc = ac.parity_scene(*size)
    for md, scene, index, c in ((sc["depth"], sc["scene"], sc["index"], 0.0), (None, None, None, 0.0),
                                (sc["depth"], None, None, 0.5), (None, sc["scene"], sc["index"], 0.0)):
        want = A.project_keypoints(sc["poses"], sc["kp"], sc["K"], size, md, scene, index, pixel_center=c)
        got = device_keypoints(sc, md, scene, index, c)
        assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
        assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
        assert np.array_equal(got[2], want[2])
    # the scene is what it claims: hidden and visible, known and missing, outside and behind all occur
    fl = A.project_keypoints(sc["poses"], sc["kp"], sc["K"], size, sc["depth"], sc["scene"], sc["index"])[2]
    assert (fl[4] == 0).all() and (fl[2] == ac.FRONT).all()
    assert ((fl[:2] & ac.SELF) == 0).any() and (fl[:2] & ac.SELF).any()
    assert ((fl[[0, 1, 3]] & ac.IN_IMAGE) != 0).any() and ((fl[3] & ac.IN_IMAGE) == 0).any()
    # and the public wrapper on the device gives the same
    dev = A.project_keypoints(sc["poses"], sc["kp"], sc["K"], size, sc["depth"], sc["scene"], sc["index"], device="cuda")
    assert np.array_equal(dev[2], fl)


@pytest.mark.parametrize("size", SIZES)
def test_mask_boxes_parity(size):
    import torch
    from betapose_amd import _lib, annotate as A
    sc = ac.parity_scene(*size)
    H, W = size
    P = len(sc["depth"])
    Kf = np.ascontiguousarray(sc["K"]).reshape(9)
    for scene, index, c in ((sc["scene"], sc["index"], 0.0), (None, None, 0.0), (sc["scene"], sc["index"], 0.5)):
        want = A.mask_boxes(sc["depth"], sc["K"], scene, index, pixel_center=c)
        d = [_dev(sc["depth"]), _dev(scene), _dev(index)]

        def call(s):
            boxes = torch.full((P, 2, 4), FILL, dtype=torch.int32, device="cuda")
            counts = torch.full((P, 2), FILL, dtype=torch.int32, device="cuda")
            if s is not None:
                s.wait_stream(torch.cuda.current_stream())
            _lib.check(_lib.lib().bp_mask_boxes(_lib.ptr(d[0]), P, H, W, _lib.ptr(Kf), c, _lib.ptr(d[1]),
                                                0 if scene is None else len(scene), _lib.ptr(d[2]), 0.015, _lib.ptr(boxes),
                                                _lib.ptr(counts), _stream(s)))
            return boxes.cpu().numpy(), counts.cpu().numpy()
        got = _runs(call)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    boxes, counts = A.mask_boxes(sc["depth"], sc["K"], sc["scene"], sc["index"])
    assert boxes[2].tolist() == [[-1] * 4] * 2 and counts[2].tolist() == [0, 0] and boxes[4].tolist() == [[-1] * 4] * 2
    assert boxes[3, 0, 0] == 0 and 0 < counts[0, 1] < counts[0, 0]          # cut by the border; partly hidden
    if H > 16:
        assert boxes[0, 0, 3] - boxes[0, 0, 2] >= 16                        # the object spans more than one band of rows
    dev = A.mask_boxes(sc["depth"], sc["K"], sc["scene"], sc["index"], device="cuda")
    assert np.array_equal(dev[0], boxes) and np.array_equal(dev[1], counts)


@pytest.mark.parametrize("n", [500, 2048 + 37])
@pytest.mark.parametrize("size", SIZES)
def test_vertex_boxes_parity(size, n):
    import torch
    from betapose_amd import _lib, annotate as A
    sc = ac.parity_scene(*size)
    H, W = size
    cloud = sc["cloud"] if n == 500 else np.random.default_rng(n).normal(size=(n, 3)) * 0.03
    P = len(sc["poses"])
    want = A.vertex_boxes(sc["poses"], cloud, sc["K"], size)
    d = [_dev(sc["poses"].reshape(P, 12)), _dev(cloud)]
    Kf = np.ascontiguousarray(sc["K"]).reshape(9)

    def call(s):
        boxes = torch.full((P, 4), FILL, dtype=torch.int32, device="cuda")
        if s is not None:
            s.wait_stream(torch.cuda.current_stream())
        _lib.check(_lib.lib().bp_vertex_boxes(_lib.ptr(d[0]), P, _lib.ptr(d[1]), n, _lib.ptr(Kf), H, W, _lib.ptr(boxes),
                                              _stream(s)))
        return (boxes.cpu().numpy(),)
    got = _runs(call)[0]
    assert np.array_equal(got, want)
    assert want[2].tolist() == [-1] * 4 and want[3, 0] == 1 and (want[0] >= 0).all()    # empty; the strict left bound
    assert np.array_equal(A.vertex_boxes(sc["poses"], cloud, sc["K"], size, device="cuda"), want)


@pytest.mark.parametrize("res", [(80, 64), (13, 10)])
def test_kpd_targets_parity(res):
    import torch
    from betapose_amd import _lib, annotate as A
    parts, ul, br, in_res, out_res = ac.target_case(*res)
    B, Kp = parts.shape[:2]
    want = A.kpd_targets(parts, ul, br, in_res, out_res, want_mask=True)
    g = A.gaussian_table(1)
    d = [_dev(parts), _dev(ul), _dev(br), _dev(g)]
    for with_mask in (True, False):
        def call(s):
            out = torch.full((B, Kp) + res, float(FILL), dtype=torch.float32, device="cuda")
            centres = torch.full((B, Kp, 2), FILL, dtype=torch.int32, device="cuda")
            mask = torch.full((B, Kp) + res, float(FILL), dtype=torch.float32, device="cuda") if with_mask else None
            if s is not None:
                s.wait_stream(torch.cuda.current_stream())
            _lib.check(_lib.lib().bp_kpd_targets(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), B, Kp, in_res[0], in_res[1], res[0],
                                                 res[1], _lib.ptr(d[3]), len(g), _lib.ptr(out), _lib.ptr(centres), _lib.ptr(mask),
                                                 _stream(s)))
            if s is not None:
                s.synchronize()
            torch.cuda.synchronize()
            return (out.cpu().numpy(), centres.cpu().numpy()) + ((mask.cpu().numpy(),) if with_mask else ())
        got = _runs(call)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
        if with_mask:
            assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert (want[1][:, 4] == -1).all() and not want[0][:, 4].any() and (want[0][0, 1] > 0).sum() < 49     # undrawn; clipped
    dev = A.kpd_targets(parts, ul, br, in_res, out_res, device="cuda")
    assert np.array_equal(dev[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(dev[1], want[1])


def test_kpd_targets_unaligned_output():
    """An output tensor that starts 4 bytes past a 16-byte boundary takes the scalar stores everywhere: same maps."""
    import torch
    from betapose_amd import _lib, annotate as A
    parts, ul, br, in_res, res = ac.target_case(80, 64)
    B, Kp = parts.shape[:2]
    want = A.kpd_targets(parts, ul, br, in_res, res)
    g = A.gaussian_table(1)
    d = [_dev(parts), _dev(ul), _dev(br), _dev(g)]
    count = B * Kp * res[0] * res[1]
    buf = torch.full((count + 2,), float(FILL), dtype=torch.float32, device="cuda")
    centres = torch.full((B, Kp, 2), FILL, dtype=torch.int32, device="cuda")
    out = buf[1:count + 1]
    assert out.data_ptr() % 16 == 4
    _lib.check(_lib.lib().bp_kpd_targets(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), B, Kp, in_res[0], in_res[1], res[0], res[1],
                                         _lib.ptr(d[3]), len(g), out.data_ptr(), _lib.ptr(centres), None,
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[0] == FILL and got[-1] == FILL                                # nothing outside the tensor is touched
    assert np.array_equal(got[1:-1].view(np.uint32), want[0].reshape(-1).view(np.uint32))


def test_device_refuses_a_scene_index_out_of_range():
    import torch
    from betapose_amd import _lib
    sc = ac.parity_scene(37, 70)
    P, Kp = len(sc["poses"]), len(sc["kp"])
    bad = sc["index"].copy()
    bad[3] = 2
    d = [_dev(sc["poses"].reshape(P, 12)), _dev(sc["kp"]), _dev(sc["scene"]), _dev(bad)]
    xy = torch.zeros((P, Kp, 2), dtype=torch.float64, device="cuda")
    z = torch.zeros((P, Kp), dtype=torch.float64, device="cuda")
    fl = torch.zeros((P, Kp), dtype=torch.uint8, device="cuda")
    lib = _lib.lib()
    rc = lib.bp_annotate_keypoints(_lib.ptr(d[0]), P, _lib.ptr(d[1]), Kp, _lib.ptr(np.ascontiguousarray(sc["K"]).reshape(9)), 37, 70,
                                   0.0, 0.01, None, _lib.ptr(d[2]), 2, _lib.ptr(d[3]), 0.015, 0.015, _lib.ptr(xy), _lib.ptr(z),
                                   _lib.ptr(fl), torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b"scene index" in lib.bp_last_error()
    boxes = torch.zeros((P, 2, 4), dtype=torch.int32, device="cuda")
    counts = torch.zeros((P, 2), dtype=torch.int32, device="cuda")
    rc = lib.bp_mask_boxes(_lib.ptr(_dev(sc["depth"])), P, 37, 70, _lib.ptr(np.ascontiguousarray(sc["K"]).reshape(9)), 0.0,
                           _lib.ptr(d[2]), 2, _lib.ptr(d[3]), 0.015, _lib.ptr(boxes), _lib.ptr(counts),
                           torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b"scene index" in lib.bp_last_error()


def test_annotate_sequence_device_equals_host(tmp_path):
    from betapose_amd import annotate as A
    sys.path.insert(0, ac.ROOT)
    sys.path.insert(0, os.path.join(ac.ROOT, "tests"))
    import annotate as cli
    from test_annotate_host import write_tree
    base = str(tmp_path / "sixd")
    write_tree(base, frames=3)
    bench, kp3d, faces, size = cli.load_bench(base, 1, 12, True, True)
    for kw in ({"faces": faces, "use_depth": True}, {"reference": True}):
        host = A.annotate_sequence(bench, 1, kp3d, **kw)
        dev = A.annotate_sequence(bench, 1, kp3d, device="cuda", **kw)
        assert set(host) == set(dev)
        for k in host:
            assert np.array_equal(host[k].view(np.uint8), dev[k].view(np.uint8)), k
