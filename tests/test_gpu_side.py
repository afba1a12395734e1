"""``_lib.Side`` on a device: the call goes to the current stream of its device, and ``put`` moves what it must."""
import numpy as np
import pytest

from betapose_amd import _lib

pytestmark = pytest.mark.gpu


def _overlay(side, frames, color, depth, alpha=77):
    out = side.empty(frames.shape, np.uint8)
    I, H, W = depth.shape
    side.call("bp_overlay", side.put(frames), side.put(color), side.put(depth), I, H, W, alpha, out)
    return out


def test_side_device_matches_host(cuda):
    import torch
    rng = np.random.default_rng(5)
    frames, color = rng.integers(0, 256, (2, 3, 5, 3), np.uint8), rng.integers(0, 256, (2, 3, 5, 3), np.uint8)
    depth = (rng.random((2, 3, 5)) * (rng.random((2, 3, 5)) < 0.6)).astype(np.float32)
    host, side = _lib.Side(), _lib.Side(cuda)
    want = host.get(_overlay(host, frames, color, depth))
    assert side.dev == cuda and (want != frames).any()
    got = side.get(_overlay(side, frames, color, depth))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    stream = torch.cuda.Stream(cuda)
    with torch.cuda.stream(stream):
        out = _overlay(side, frames, color, depth)
    stream.synchronize()
    assert np.array_equal(side.get(out), want)


def test_side_device_put(cuda):
    import torch
    side = _lib.Side(cuda)
    t = torch.arange(12, dtype=torch.float32, device=cuda).reshape(3, 4)
    assert side.put(t).data_ptr() == t.data_ptr() and side.put(t, np.float32).data_ptr() == t.data_ptr()
    assert side.put(None) is None
    u = np.array([0, 1, 0x7FFF, 0x8000, 0xFFFF], np.uint16)
    u.setflags(write=False)
    d = side.put(u)
    assert d.dtype == torch.int16 and d.device == cuda
    back = side.get(d, np.uint16)
    assert back.dtype == np.uint16 and np.array_equal(back, u)
    z = side.zeros((2, 3), np.uint64)
    assert z.dtype == torch.int64 and not side.get(z, np.uint64).any()
