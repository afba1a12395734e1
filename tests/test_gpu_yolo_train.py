"""The detector-training kernels (csrc/yolo_train.hip: bp_yolo_inputs, bp_yolo_truth, bp_yolo_loss) against their host
twins, bit for bit: uint32 / uint64 views of the floats, array_equal of the integers.  Frames of 37 x 70 and 480 x 640,
network inputs of 24 x 16, 13 x 10 (width % 4 != 0: the scalar-store path) and 416 x 416 once, an output offset by one
float, B = 4 with flipped and unflipped, distorted and identity-distorted samples and one out-of-range frame index in one
batch; the golden archive's truth cases as one batch; the loss on the archive's cases (grids 3 x 2, 5 x 7, 13 x 13, classes
1 and 3) and once at 52 x 52, the only grid with more cells than one block.  Every output buffer is pre-filled with a
sentinel; every function runs twice and once on a second stream.  Then YoloSampleLoader on the device against the same
loader on the host twins, and YoloLoss's backward on the device against the host's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import yolo_train_common as yc  # noqa: E402

FILL = 113.0


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream(s):
    import torch
    return (s if s is not None else torch.cuda.current_stream()).cuda_stream


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


def _sentinel(shape, offset=0, dtype=None):
    """a sentinel-filled tensor of ``shape``; offset = 1: a view that starts one element into its buffer (not 16-byte aligned)"""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + offset,), FILL, dtype=dtype or torch.float32, device="cuda")
    return buf[offset:].view(*shape)


def _on(s, launch, outs):
    import torch
    if s is not None:
        s.wait_stream(torch.cuda.current_stream())
    launch(_stream(s))
    if s is not None:
        s.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def device_inputs(frames, idx, crop, flip, hsv, net, offset=0):
    from betapose_amd import _lib
    N, H, W = frames.shape[:3]
    B = len(idx)
    d = [_dev(frames), _dev(idx), _dev(crop), _dev(flip), _dev(hsv)]

    def call(s):
        out = _sentinel((B, 3, net[0], net[1]), offset)
        return _on(s, lambda st: _lib.check(_lib.lib().bp_yolo_inputs(_lib.ptr(d[0]), N, H, W, *(_lib.ptr(a) for a in d[1:]), B, net[0],
                                                                      net[1], out.data_ptr(), st)), (out,))
    return _runs(call)[0]


def _input_case(H, W):
    frames = yc.frames_of(H, W)
    idx, crop, flip, hsv = yc.mixed_batch(H, W)
    idx = np.append(idx, 7).astype(np.int32)            # out of range: a zero sample
    return frames, idx, np.concatenate([crop, crop[:1]]), np.append(flip, 0).astype(np.uint8), np.concatenate([hsv, hsv[:1]])


@pytest.mark.parametrize("size", [(37, 70), (480, 640)])
@pytest.mark.parametrize("net", [(24, 16), (13, 10)])
def test_inputs_parity(size, net):
    from betapose_amd import yolo_train as Y
    frames, idx, crop, flip, hsv = _input_case(*size)
    for h in (hsv, None):
        want = Y.yolo_inputs(frames, idx, crop, flip, h, net)
        got = device_inputs(frames, idx, crop, flip, h, net)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert not got[3].any() and got[0].any() and got[1].any() and got[2].any()


@pytest.mark.parametrize("net", [(24, 16), (13, 10)])
def test_inputs_unaligned_output(net):
    """an output tensor that starts one float into its buffer: every row takes the scalar-store path"""
    from betapose_amd import yolo_train as Y
    frames, idx, crop, flip, hsv = _input_case(37, 70)
    want = Y.yolo_inputs(frames, idx, crop, flip, hsv, net)
    got = device_inputs(frames, idx, crop, flip, hsv, net, offset=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_inputs_full_resolution_and_wrapper():
    from betapose_amd import yolo_train as Y
    frames, idx, crop, flip, hsv = _input_case(480, 640)
    sel = [0, 1, 2]
    want = Y.yolo_inputs(frames, idx[sel], crop[sel], flip[sel], hsv[sel], (416, 416))
    got = device_inputs(frames, idx[sel], crop[sel], flip[sel], hsv[sel], (416, 416))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    dev = Y.yolo_inputs(frames, idx[sel], crop[sel], flip[sel], hsv[sel], (416, 416), device="cuda")
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_inputs_against_the_reference_on_the_device():
    from betapose_amd import yolo_train as Y
    for c in yc.meta()["image_cases"]:
        args, _ = yc.image_case(c)
        assert np.array_equal(Y.yolo_inputs(*args, device="cuda").cpu().numpy().view(np.uint32), Y.yolo_inputs(*args).view(np.uint32))


def test_inputs_argument_error_on_the_device():
    from betapose_amd import _lib
    from betapose_amd import yolo_train as Y
    frames, idx, crop, flip, hsv = _input_case(37, 70)
    bad = crop.copy()
    bad[1, 2] = 1
    with pytest.raises(_lib.BetaposeHipError):
        Y.yolo_inputs(frames, idx, bad, flip, hsv, (24, 16), device="cuda")


def test_truth_parity():
    import torch
    from betapose_amd import _lib
    from betapose_amd import yolo_train as Y
    labels, first, swap, geom, flip, classes, max_boxes, net = yc.truth_batch()
    B, M = len(first) - 1, len(labels)
    want_t, want_k = Y.yolo_truth(labels, first, swap, geom, flip, classes, max_boxes, net)
    d = [_dev(labels), _dev(first), _dev(swap), _dev(geom), _dev(flip)]

    def call(s):
        order = _sentinel((M,), dtype=torch.int32)
        truth, kept = _sentinel((B, max_boxes, 5)), _sentinel((B,), dtype=torch.int32)
        return _on(s, lambda st: _lib.check(_lib.lib().bp_yolo_truth(_lib.ptr(d[0]), M, *(_lib.ptr(a) for a in d[1:]), B, classes,
                                                                     max_boxes, net[1], net[0], 0, order.data_ptr(), truth.data_ptr(),
                                                                     kept.data_ptr(), st)), (truth, kept))
    truth, kept = _runs(call)
    assert np.array_equal(truth.view(np.uint32), want_t.view(np.uint32)) and np.array_equal(kept, want_k)
    assert kept[0] == 0 and kept.max() >= 80 and truth.any()
    t2, k2 = Y.yolo_truth(labels, first, swap, geom, flip, classes, max_boxes, net, device="cuda")
    assert np.array_equal(t2.cpu().numpy().view(np.uint32), want_t.view(np.uint32)) and np.array_equal(k2.cpu().numpy(), want_k)
    # a batch without a label
    t3, k3 = Y.yolo_truth(np.zeros((0, 5), np.float32), np.zeros(3, np.int32), np.zeros(0, np.int32), geom[:2], flip[:2], device="cuda")
    assert not t3.cpu().numpy().any() and k3.cpu().tolist() == [0, 0]


def device_loss(x, truth, kw, want_act=True):
    import torch
    from betapose_amd import _lib
    B, C, h, w = x.shape
    n, classes = len(kw["mask"]), kw["classes"]
    d = [_dev(x), _dev(kw["anchors"]), _dev(kw["mask"]), _dev(truth)]
    parts = int(_lib.lib().bp_yolo_loss_partials(B, n, classes, h, w))

    def call(s):
        act = _sentinel(x.shape) if want_act else None
        delta = _sentinel(x.shape)
        cost, stats = _sentinel((1,), dtype=torch.float64), _sentinel((7,), dtype=torch.float64)
        partial = _sentinel((parts,), dtype=torch.float64)
        launch = lambda st: _lib.check(_lib.lib().bp_yolo_loss(
            _lib.ptr(d[0]), B, C, n, classes, h, w, kw["net_size"][1], kw["net_size"][0], _lib.ptr(d[1]), len(kw["anchors"]), _lib.ptr(d[2]),
            _lib.ptr(d[3]), truth.shape[1], kw["ignore_thresh"], kw["truth_thresh"], 0, None if act is None else act.data_ptr(),
            delta.data_ptr(), cost.data_ptr(), stats.data_ptr(), partial.data_ptr(), st))
        return _on(s, launch, (delta, cost, stats) + ((act,) if want_act else ()))
    return _runs(call)


def _loss_parity(x, truth, kw):
    from betapose_amd import yolo_train as Y
    cost, st, delta, act = Y.yolo_loss(x, truth, **kw)
    got = device_loss(x, truth, kw)
    assert np.array_equal(got[0].view(np.uint32), delta.view(np.uint32)) and np.array_equal(got[3].view(np.uint32), act.view(np.uint32))
    assert np.array_equal(got[1].view(np.uint64), np.array([cost]).view(np.uint64))
    assert np.array_equal(got[2].view(np.uint64), np.array([st[k] for k in Y.STAT_NAMES]).view(np.uint64))
    assert delta.any() and st["count"] > 0
    return cost


@pytest.mark.parametrize("grid", ["g3x2", "g5x7", "g13x13"])
def test_loss_parity_on_the_fixture(grid):
    cases = [c for c in yc.meta()["loss_cases"] if c["name"].startswith(grid)]
    assert cases and (grid == "g13x13" or {c["classes"] for c in cases} == {1, 3})
    for c in cases:
        x, truth, kw, _, _ = yc.loss_case(c)
        _loss_parity(x, truth, kw)


def test_loss_parity_over_several_blocks_and_wrapper():
    from betapose_amd import yolo_train as Y
    mask = np.array([0, 1, 2], np.int32)
    x, truth = yc.synthetic_loss(52, 52, 3, mask)
    kw = dict(net_size=(yc.NET, yc.NET), anchors=np.array(yc.golden()["anchors"]), mask=mask, classes=3, ignore_thresh=0.7, truth_thresh=1.0)
    cost = _loss_parity(x, truth, kw)
    got = device_loss(x, truth, kw, want_act=False)
    assert np.array_equal(got[1].view(np.uint64), np.array([cost]).view(np.uint64))
    c2, st2, d2, a2 = Y.yolo_loss(x, truth, device="cuda", **kw)
    assert c2 == cost and d2.is_cuda and a2.is_cuda


def test_loader_on_the_device_equals_the_host(tmp_path):
    from betapose_amd import yolo_train as Y
    lst = yc.write_folder(str(tmp_path / "set"), n=5)
    host = list(Y.YoloSampleLoader(lst, 2, net_size=(24, 32), seed=3))
    dev = list(Y.YoloSampleLoader(lst, 2, net_size=(24, 32), seed=3, device="cuda"))
    assert len(host) == len(dev) == 3
    for (hi, ht), (di, dt) in zip(host, dev):
        assert di.is_cuda and dt.is_cuda
        assert np.array_equal(di.cpu().numpy().view(np.uint32), hi.view(np.uint32))
        assert np.array_equal(dt.cpu().numpy().view(np.uint32), ht.view(np.uint32)) and ht.any()


def test_yolo_loss_backward_on_the_device_equals_the_host():
    import torch
    from betapose_amd import yolo_train as Y
    c = [k for k in yc.meta()["loss_cases"] if k["name"] == "g5x7_c3_m1"][0]
    x, truth, kw, _, _ = yc.loss_case(c)
    args = (kw["net_size"], kw["anchors"], kw["mask"], kw["classes"], kw["ignore_thresh"], kw["truth_thresh"])
    grads = []
    for dev in ("cpu", "cuda"):
        xt = torch.from_numpy(x).to(dev).requires_grad_(True)
        loss = Y.YoloLoss.apply(xt, torch.from_numpy(truth).to(dev), *args)
        (2 * loss).backward()
        grads.append((float(loss.detach()), xt.grad.cpu().numpy()))
    assert grads[0][0] == grads[1][0] and np.array_equal(grads[0][1].view(np.uint32), grads[1][1].view(np.uint32))
    _, _, delta, _ = Y.yolo_loss(x, truth, **kw)
    assert np.array_equal(grads[1][1], -2 * delta)
