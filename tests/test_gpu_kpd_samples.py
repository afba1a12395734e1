"""The KPD training-sample kernels (csrc/kpd_sample.hip: bp_kpd_inputs, bp_kpd_augment, bp_heatmap_loss_acc) against their
host twins, bit for bit: uint32 / uint64 views of the floats, array_equal of the integers.  Frames of 37 x 70 (W neither a
multiple of 64 nor of 4) and 480 x 640, inputs of 20 x 16, 13 x 10 (inpW % 4 != 0) and 320 x 256, an output offset by one
float (the scalar-store path), B = 3, Kp = 7, rotations mixed with unrotated and unflipped samples in one batch, the loss at
13 x 10 and 80 x 64 with and without mask and gradient.  Every output buffer is pre-filled with a sentinel; every
function runs twice and once on a second stream.  Then HeatmapMSE's backward through a one-layer conv against
torch.nn.MSELoss, and KPDSampleLoader on the device against the same loader on the host twins."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kpd_samples_common as kc  # noqa: E402

FILL = 113.0


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


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


def device_inputs(frames, idx, ul, br, gains, blank, res, offset=0):
    import torch
    from betapose_amd import _lib
    N, H, W = frames.shape[:3]
    B = len(idx)
    d = [_dev(frames), _dev(np.asarray(idx, np.int32)), _dev(ul), _dev(br), _dev(gains), _dev(blank)]

    def call(s):
        inp = _sentinel((B, 3, res[0], res[1]), offset)
        if s is not None:
            s.wait_stream(torch.cuda.current_stream())
        _lib.check(_lib.lib().bp_kpd_inputs(_lib.ptr(d[0]), N, H, W, *(_lib.ptr(a) for a in d[1:]), B, res[0], res[1],
                                            inp.data_ptr(), _stream(s)))
        if s is not None:
            s.synchronize()
        return (inp.cpu().numpy(),)
    return _runs(call)[0]


def _input_case(H, W):
    frames = kc.frames_of(H, W)
    ul, br = kc.window_cases(H, W)
    B = len(ul)
    idx = np.arange(B, dtype=np.int32) % 2
    gains = np.random.default_rng(1).uniform(0.7, 1.3, (B, 3)).astype(np.float32)
    gains[0], gains[1] = (0.7, 1.3, 0.7), (1.3, 0.7, 1.3)
    blank = np.zeros(B, np.uint8)
    blank[5] = 1
    return frames, idx, ul, br, gains, blank


@pytest.mark.parametrize("size", [(37, 70), (480, 640)])
@pytest.mark.parametrize("res", [(20, 16), (13, 10)])
def test_inputs_parity(size, res):
    from betapose_amd import train_data as T
    frames, idx, ul, br, gains, blank = _input_case(*size)
    for g in (gains, None):
        want = T.kpd_inputs(frames, idx, ul, br, g, blank, res)
        got = device_inputs(frames, idx, ul, br, g, blank, res)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert not got[5].any() and got[0].any()
    ones = device_inputs(frames, idx, ul, br, np.ones_like(gains), blank, res)       # a gain of 1.0f changes no bit
    assert np.array_equal(ones.view(np.uint32), want.view(np.uint32))


def test_inputs_full_resolution_and_wrapper():
    from betapose_amd import train_data as T
    frames, idx, ul, br, gains, blank = _input_case(480, 640)
    sel = [0, 3]
    want = T.kpd_inputs(frames, idx[sel], ul[sel], br[sel], gains[sel], None, (320, 256))
    got = device_inputs(frames, idx[sel], ul[sel], br[sel], gains[sel], None, (320, 256))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    dev = T.kpd_inputs(frames, idx[sel], ul[sel], br[sel], gains[sel], None, (320, 256), device="cuda")
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("res", [(20, 16), (13, 10)])
def test_inputs_unaligned_output(res):
    """an output tensor that starts one float into its buffer: every row takes the scalar-store path"""
    from betapose_amd import train_data as T
    frames, idx, ul, br, gains, blank = _input_case(37, 70)
    want = T.kpd_inputs(frames, idx, ul, br, gains, blank, res)
    got = device_inputs(frames, idx, ul, br, gains, blank, res, offset=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def device_augment(x, flip, cs, perm, offset=0):
    import torch
    from betapose_amd import _lib
    B, C, H, W = x.shape
    d = [_dev(x), _dev(flip), _dev(cs), _dev(perm)]

    def call(s):
        y = _sentinel(x.shape, offset)
        if s is not None:
            s.wait_stream(torch.cuda.current_stream())
        _lib.check(_lib.lib().bp_kpd_augment(_lib.ptr(d[0]), B, C, H, W, _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), y.data_ptr(),
                                             _stream(s)))
        if s is not None:
            s.synchronize()
        return (y.cpu().numpy(),)
    return _runs(call)[0]


@pytest.mark.parametrize("shape", [(5, 3, 20, 16), (5, 7, 13, 10), (5, 7, 80, 64)])
@pytest.mark.parametrize("offset", [0, 1])
def test_augment_parity(shape, offset):
    """angles 0, 17.3, -63 and 80 mixed within one batch with unrotated and unflipped samples"""
    from betapose_amd import train_data as T
    x = np.random.default_rng(4).uniform(-0.55, 0.55, shape).astype(np.float32)
    flip = np.array([1, 0, 1, 0, 1], np.uint8)
    angle = np.array([0.0, 17.3, -63.0, 0.0, 80.0])
    pairs = kc.FLIP_PAIRS if shape[1] == 7 else ()
    want = T.augment_maps(x, flip, angle, pairs)
    perm = T.channel_table(shape[1], pairs) if pairs else None
    got = device_augment(x, flip, T.rotation_terms(angle), perm, offset)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[3], x[3]) and not np.array_equal(got[1], x[1])
    if offset == 0:
        dev = T.augment_maps(_dev(x), flip, angle, pairs, device="cuda")
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy().view(np.uint32), want.view(np.uint32))


def device_loss(out, lab, mask, want_grad, offset=0):
    import torch
    from betapose_amd import _lib
    B, K, H, W = out.shape
    d = [_dev(out), _dev(lab), _dev(mask)]

    def call(s):
        partial = _sentinel((B * K,), dtype=torch.float64)
        loss = _sentinel((1,), dtype=torch.float64)
        acc, dists = _sentinel((K + 1,)), _sentinel((K, B))
        preds, gt = _sentinel((B, K, 2), dtype=torch.int32), _sentinel((B, K, 2), dtype=torch.int32)
        grad = _sentinel(out.shape, offset) if want_grad else None
        if s is not None:
            s.wait_stream(torch.cuda.current_stream())
        _lib.check(_lib.lib().bp_heatmap_loss_acc(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), B, K, H, W, _lib.ptr(partial),
                                                  _lib.ptr(loss), _lib.ptr(acc), _lib.ptr(preds), _lib.ptr(gt), _lib.ptr(dists),
                                                  None if grad is None else grad.data_ptr(), _stream(s)))
        if s is not None:
            s.synchronize()
        res = [loss.cpu().numpy(), acc.cpu().numpy(), preds.cpu().numpy(), gt.cpu().numpy(), dists.cpu().numpy()]
        return tuple(res + ([grad.cpu().numpy()] if want_grad else []))
    return _runs(call)


@pytest.mark.parametrize("res", [(13, 10), (80, 64)])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("want_grad", [False, True])
def test_loss_parity(res, masked, want_grad):
    from betapose_amd import train_data as T
    out, lab, mask = kc.heat_batch(3, 7, *res)
    mask = mask if masked else None
    want = T.heatmap_loss_accuracy(out, lab, mask, want_grad)
    got = device_loss(out, lab, mask, want_grad)
    assert got[0].view(np.uint64)[0] == np.float64(want[0]).view(np.uint64)
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.array_equal(got[4].view(np.uint32), want[4].view(np.uint32))
    assert got[2][0, 0].tolist() == [res[1] - 3, 3]                               # the tie goes to the lower flat index
    assert (got[4][5] == -1).all() and got[1][6] == -1 and got[4][2, 1] == -1
    if want_grad:
        assert np.array_equal(got[5].view(np.uint32), want[5].view(np.uint32))
        odd = device_loss(out, lab, mask, True, offset=1)                         # an unaligned gradient: scalar loads and stores
        assert odd[0].view(np.uint64)[0] == got[0].view(np.uint64)[0] and np.array_equal(odd[5].view(np.uint32), want[5].view(np.uint32))
    w = T.heatmap_loss_accuracy(out, lab, mask, want_grad, device="cuda")
    assert np.float64(w[0]).view(np.uint64) == np.float64(want[0]).view(np.uint64) and np.array_equal(w[1], want[1])


def test_loss_threshold_case():
    from betapose_amd import train_data as T
    out, lab, mask = kc.threshold_batch()
    want = T.heatmap_loss_accuracy(out, lab, mask)
    got = device_loss(out, lab, mask, False)
    assert got[0].view(np.uint64)[0] == np.float64(want[0]).view(np.uint64)
    for a, b in zip(got[1:], want[1:5]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert got[4][0, 0] == 0.5 and got[4][0, 1] > 0.5 and got[1][1] == 0.5


def test_heatmap_mse_backward():
    """backward through a one-layer 1 x 1 conv on the device: weight.grad against the same graph under
    torch.nn.MSELoss.  Tolerance 1e-5 relative to the largest gradient: float32 accumulation of a 1 x 1 conv over 130
    pixels."""
    import torch
    from betapose_amd import train_data as T
    torch.manual_seed(0)
    x = torch.randn(3, 4, 13, 10, device="cuda")
    lab = torch.rand(3, 7, 13, 10, device="cuda")
    mask = torch.ones_like(lab)
    mask[1, 2] = 0
    grads = []
    for crit in (lambda o: T.HeatmapMSE.apply(o, lab, mask), lambda o: torch.nn.MSELoss()(o * mask, lab)):
        torch.manual_seed(1)
        conv = torch.nn.Conv2d(4, 7, 1).cuda()
        loss = crit(conv(x))
        (loss * 3.0).backward()
        grads.append((float(loss), conv.weight.grad.cpu().numpy().copy(), conv.bias.grad.cpu().numpy().copy()))
    (l0, w0, b0), (l1, w1, b1) = grads
    print("HeatmapMSE loss %.9g vs MSELoss %.9g; weight.grad differs by %.3g of its largest" % (l0, l1, np.abs(w0 - w1).max() / np.abs(w1).max()))
    assert abs(l0 - l1) <= 1e-6 * l1
    assert np.abs(w0 - w1).max() <= 1e-5 * np.abs(w1).max() and np.abs(b0 - b1).max() <= 1e-5 * np.abs(b1).max()
    assert T.HeatmapMSE.last["acc"].shape == (8,) and T.HeatmapMSE.last["preds"].is_cuda


def test_loader_device_equals_host(tmp_path):
    from betapose_amd import train_data as T
    annot = kc.write_folder(str(tmp_path))
    kw = dict(train=True, seed=6, add_dpg=True, in_res=(20, 16), out_res=(10, 8), flip_pairs=kc.FLIP_PAIRS)
    host = list(T.KPDSampleLoader(annot, str(tmp_path), 2, **kw))
    dev = list(T.KPDSampleLoader(annot, str(tmp_path), 2, device="cuda", **kw))
    assert len(host) == len(dev) == 2
    for h, d in zip(host, dev):
        for a, b in zip(h, d):
            assert b.is_cuda and np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert host[0][0].any() and host[0][1].any()
