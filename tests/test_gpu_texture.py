"""bp_texture_mips and bp_render_color_textured (csrc/raster_texture.hip) against their host twins, byte for byte: the
cases of texture_common.py at both image sizes, several poses per image, on a stream of the caller's, and the
synthesiser with a textured target on the device."""
import numpy as np
import pytest
import torch

import texture_common as tc
from betapose_amd import metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same_bytes(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, k, int((a != b).sum()))


@pytest.mark.parametrize("size", tc.SIZES)
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_device_equals_host(name, size):
    """Colour, depth and skipped of every case (identity, flat, minification, perspective, wrap and wild coordinates,
    accumulation in both orders with three poses into two images, the exact tie)."""
    same_bytes(tc.CASES[name](DEV, size), tc.host(name, size), name)


@pytest.mark.parametrize("name", ["perspective-0.5", "wrap-bad", "into-textured-last"])
def test_device_equals_host_on_a_stream_of_the_callers(name):
    size = tc.SIZES[0]
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        got = tc.CASES[name](DEV, size)
    stream.synchronize()
    same_bytes(got, tc.host(name, size), name)


@pytest.mark.parametrize("Wt,Ht", tc.TEXTURE_SIZES + [(33, 65)])
def test_device_pyramid_equals_host(Wt, Ht):
    tex = tc.random_texture(Wt, Ht)
    host, dev = metrics.texture_mips(tex), metrics.texture_mips(tex, DEV)
    assert (dev.Wt, dev.Ht, dev.levels) == (host.Wt, host.Ht, host.levels) and dev.data.device == torch.device(DEV)
    assert np.array_equal(dev.data.cpu().numpy().view(np.uint32), host.data)


def test_one_pyramid_serves_many_calls():
    """A pyramid built once on the device, used with and without mip-mapping, equals the calls that build their own."""
    size = tc.SIZES[0]
    v, f, uv, pose = tc.tilted_quad(size)
    import raster_common as rc
    K = rc.camera(size)
    mips = metrics.texture_mips(tc.gradient_texture(), DEV)
    for mip in (True, False):
        got = metrics.render_color(pose[None], v, f, None, K, size, DEV, light=tc.LIGHT, uv=uv, texture=mips, mip=mip)
        want = metrics.render_color(pose[None], v, f, None, K, size, None, light=tc.LIGHT, uv=uv, texture=tc.gradient_texture(), mip=mip)
        same_bytes(got, want, mip)


@pytest.mark.parametrize("kind", ["scenes", "multi"])
def test_synthesiser_on_the_device_equals_host(kind):
    want = tc.host_synth(kind, True)
    got = (tc.synth_scenes if kind == "scenes" else tc.synth_multi)(True, device=DEV)
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
