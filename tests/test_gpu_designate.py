"""The key-point designator's kernels (csrc/designate.hip: bp_sift_octave, bp_farthest_points, bp_thin_points) against
their host twins, bit for bit: uint64 views of the floats, array_equal of the integers.  Clouds of 30 (below one wave),
65 (one past a wave), 300 (several tiles of q, a ragged last one, three duplicated points) and 1215 points (the scene's
first octave); k = 25 and k = 40 > n; 4, 6 and 8 scales.  Every output buffer is pre-filled with a sentinel; every
function runs twice and once on a second stream."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import designate_common as dc  # noqa: E402

FILL = 113


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared clouds are read-only)


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


def _cloud(n):
    if n == 1215:
        return dc.octave_clouds()[0][0]
    return dc.with_duplicates(n) if n == 300 else dc.nearest_part(n)


def device_octave(pts, field, scales, k, min_contrast):
    import torch
    from betapose_amd import _lib
    n, ns = len(pts), len(scales)
    d_pts = _dev(pts)
    sc = np.ascontiguousarray(scales, dtype=np.float64)

    def call(s):
        dog = torch.full((n, ns - 1), float(FILL), dtype=torch.float64, device="cuda")
        fl = torch.full((n, ns - 3), FILL, dtype=torch.int8, device="cuda")
        if s is not None:
            s.wait_stream(torch.cuda.current_stream())
        _lib.check(_lib.lib().bp_sift_octave(_lib.ptr(d_pts), n, field, _lib.ptr(sc), ns, k, min_contrast, _lib.ptr(dog),
                                             _lib.ptr(fl), _stream(s)))
        if s is not None:
            s.synchronize()
        return dog.cpu().numpy(), fl.cpu().numpy()
    return _runs(call)


@pytest.mark.parametrize("n,k,ns", [(30, 25, 6), (30, 40, 6), (65, 25, 4), (65, 25, 8), (300, 25, 6), (300, 25, 8),
                                    (1215, 25, 6)])
def test_sift_octave_parity(n, k, ns):
    from betapose_amd import designate as D
    pts = _cloud(n)
    scales = D.octave_scales(1.0, 0, ns - 3)
    want_dog, want_flags = D.sift_octave(pts, 2, scales, k, 0.02)
    dog, flags = device_octave(pts, 2, scales, k, 0.02)
    assert np.array_equal(dog.view(np.uint64), want_dog.view(np.uint64))
    assert np.array_equal(flags, want_flags)
    if n == 1215:       # the scene is what it claims: extrema of both signs
        assert (flags == 1).any() and (flags == -1).any()
        # and another field and the public wrapper on the device give the host's too
        dev = D.sift_octave(pts, 0, scales, k, 0.02, device="cuda")
        host = D.sift_octave(pts, 0, scales, k, 0.02)
        assert np.array_equal(dev[0].view(np.uint64), host[0].view(np.uint64)) and np.array_equal(dev[1], host[1])


@pytest.mark.parametrize("octave", [1, 2])
def test_sift_octave_parity_on_the_coarser_octaves(octave):
    from betapose_amd import designate as D
    pts, scales = dc.octave_clouds()[octave]
    want_dog, want_flags = D.sift_octave(pts, 2, scales, 25, 0.02)
    dog, flags = device_octave(pts, 2, scales, 25, 0.02)
    assert np.array_equal(dog.view(np.uint64), want_dog.view(np.uint64))
    assert np.array_equal(flags, want_flags)
    assert (flags == 1).any() and (flags == -1).any()


@pytest.mark.parametrize("n", [65, 1215])
@pytest.mark.parametrize("K", [1, 8, 50])
def test_farthest_points_parity(n, K):
    import torch
    from betapose_amd import _lib, designate as D
    pts = _cloud(n) if n != 65 else dc.with_duplicates(65)
    d_pts = _dev(pts)
    for start in (-1, 7):
        want = D.farthest_points(pts, K, None if start < 0 else start)

        def call(s):
            idx = torch.full((K,), FILL, dtype=torch.int32, device="cuda")
            d2 = torch.full((K,), float(FILL), dtype=torch.float64, device="cuda")
            if s is not None:
                s.wait_stream(torch.cuda.current_stream())
            _lib.check(_lib.lib().bp_farthest_points(_lib.ptr(d_pts), n, K, start, _lib.ptr(idx), _lib.ptr(d2), _stream(s)))
            return idx.cpu().numpy(), d2.cpu().numpy()
        idx, d2 = _runs(call)
        assert np.array_equal(idx, want[0])
        assert np.array_equal(d2.view(np.uint64), want[1].view(np.uint64))
    dev = D.farthest_points(pts, K, device="cuda")
    host = D.farthest_points(pts, K)
    assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1].view(np.uint64), host[1].view(np.uint64))


def _capped_cloud():
    """50 points 150 apart with three duplicated ones: three rounds delete, then the 100.0 cap stops the device loop."""
    pts = np.array(dc.far_cloud(50))
    for src, dst in ((40, 3), (20, 41), (10, 30)):
        pts[dst] = pts[src]
    return pts


@pytest.mark.parametrize("case", ["50", "257", "1000", "capped"])
def test_thin_points_parity(case):
    import torch
    from betapose_amd import _lib, designate as D
    pts = _capped_cloud() if case == "capped" else dc.thin_cloud(int(case))
    n, keep = len(pts), 30
    alive, state = np.empty(n, np.uint8), np.empty(2, np.int32)
    _lib.check(_lib.lib().bp_thin_points_host(_lib.ptr(np.ascontiguousarray(pts)), n, keep, _lib.ptr(alive), _lib.ptr(state)))
    d_pts = _dev(pts)

    def call(s):
        d_alive = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        d_state = torch.full((2,), FILL, dtype=torch.int32, device="cuda")
        if s is not None:
            s.wait_stream(torch.cuda.current_stream())
        _lib.check(_lib.lib().bp_thin_points(_lib.ptr(d_pts), n, keep, _lib.ptr(d_alive), _lib.ptr(d_state), _stream(s)))
        return d_alive.cpu().numpy(), d_state.cpu().numpy()
    got_alive, got_state = _runs(call)
    assert np.array_equal(got_alive, alive)
    assert np.array_equal(got_state, state)
    if case == "capped":
        assert state[0] == 3 and alive.sum() == n - 3       # stopped at the cap, 17 rounds early
    else:
        assert state[0] == n - keep and alive.sum() == keep
    assert np.array_equal(D.thin_points(pts, 45 if case == "capped" else keep, device="cuda"),
                          D.thin_points(pts, 45 if case == "capped" else keep))


def test_end_to_end_on_the_device():
    from betapose_amd import designate as D
    pts = dc.scene()
    host, sizes = D.sift_keypoints(pts, min_contrast=0.02, return_sizes=True, **dc.SCENE_ARGS)
    dev, dev_sizes = D.sift_keypoints(pts, min_contrast=0.02, return_sizes=True, device="cuda", **dc.SCENE_ARGS)
    assert sizes == dev_sizes == dc.OCTAVE_SIZES
    assert len(host) > 5 and np.array_equal(dev.view(np.uint64), host.view(np.uint64))
    for kw in (dict(total_kp=5, min_contrast=0.02, **dc.SCENE_ARGS), dict(total_kp=50, min_contrast=0.02, **dc.SCENE_ARGS),
               dict(total_kp=9, method="fps")):
        a, b = D.designate(pts, device="cuda", **kw), D.designate(pts, **kw)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
