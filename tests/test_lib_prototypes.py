"""The ctypes prototypes derived from include/betapose_hip.h, and the host side of ``_lib.Side`` (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import helpers
from betapose_amd import _lib

P = _lib.PROTOTYPES


def test_prototypes_cover_the_header():
    assert set(P) == helpers.header_names()


def test_prototype_types_of_known_functions():
    res, args = P["bp_yolo_loss"]
    assert res is C.c_int
    assert [i for i, a in enumerate(args) if a is C.c_float] == [14, 15]       # ignore_thresh, truth_thresh
    assert args[-1] is C.c_void_p and len(args) == 23
    assert P["bp_kpd_train_sigmoid_forward"][1] == [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    assert P["bp_synth_background"][1].count(C.c_uint) == 2
    assert P["bp_train_conv_scratch"][0] is C.c_size_t
    assert P["bp_yolo_destroy"] == (None, [C.c_void_p])
    assert P["bp_last_error"] == (C.c_char_p, [])
    assert P["bp_pipeline_frames"][0] is C.c_void_p
    assert P["bp_yolo_create"][1].count(C.c_char_p) == 2 and P["bp_yolo_create"][1][-1] is C.c_void_p
    assert P["bp_render_depth"][1][9:11] == [C.c_double, C.c_double]


def test_parser_maps_every_form():
    text = """
    /* a comment with int bp_not_this(int); inside */
    #define BP_X 1
    extern "C" {
    typedef struct bp_thing bp_thing;
    typedef struct bp_box { float x, y; } bp_box;
    const char* bp_a(void);
    void bp_b(bp_thing** out, const unsigned char* px, unsigned n, unsigned int m, long long k, size_t s, uint32_t w,
              const char* const* names, char* buf, double, float f);   // a trailing comment
    float* bp_c();
    }
    """
    assert _lib.parse_prototypes(text) == {
        "bp_a": (C.c_char_p, []),
        "bp_b": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_longlong, C.c_size_t, C.c_uint32, C.c_void_p, C.c_char_p,
                        C.c_double, C.c_float]),
        "bp_c": (C.c_void_p, [])}


@pytest.mark.parametrize("decl", ["int bp_bad(int n, real_t x);",                  # an unknown scalar type
                                  "int bp_bad(void (*done)(int, void*), void* arg);",      # a function pointer
                                  "int bp_bad(bp_box b);",                          # a struct by value
                                  "int bp_bad(const char* fmt, ...);",              # a variadic
                                  "bp_box bp_bad(int n);"])
def test_parser_refuses_what_it_cannot_map(decl):
    with pytest.raises(ValueError, match="bp_bad"):
        _lib.parse_prototypes("int bp_good(int n);\n" + decl)


def test_side_host_put():
    side = _lib.Side()
    assert side.dev is None and side.put(None) is None
    a = np.arange(24, dtype=np.float64).reshape(2, 3, 4)[:, ::2, ::-1]
    b = side.put(a, np.float32)
    assert isinstance(b, np.ndarray) and b.dtype == np.float32 and b.flags.c_contiguous and np.array_equal(b, a)
    c = np.arange(6, dtype=np.int32)
    assert side.put(c) is c and side.put(c, np.int32) is c                     # nothing to do: no copy
    d = side.put(c, copy=True)
    assert d is not c and not np.shares_memory(d, c) and np.array_equal(d, c)
    assert side.get(c) is c and not np.shares_memory(side.get(c, copy=True), c)
    z = side.zeros((2, 3), np.uint16)
    assert z.dtype == np.uint16 and z.shape == (2, 3) and not z.any()
    assert side.empty(5, np.int8).shape == (5,) and side.empty(5, np.int8).dtype == np.int8


def _overlay(side, frames, color, depth, alpha):
    out = side.empty(frames.shape, np.uint8)
    I, H, W = depth.shape
    side.call("bp_overlay", side.put(frames), side.put(color), side.put(depth), I, H, W, alpha, out)
    return side.get(out)


def test_side_host_call_overlay():
    side = _lib.Side()
    frames = np.array([[[[10, 200, 30], [0, 255, 7], [90, 91, 92]], [[1, 2, 3], [250, 128, 64], [33, 66, 99]]]], np.uint8)
    color = np.array([[[[255, 0, 100], [9, 8, 7], [0, 0, 0]], [[200, 100, 50], [5, 6, 7], [255, 255, 255]]]], np.uint8)
    depth = np.array([[[1.0, 0.0, 0.5], [0.0, 2.0, 0.0]]], np.float32)
    frames.setflags(write=False), color.setflags(write=False), depth.setflags(write=False)
    keep = frames.copy(), color.copy(), depth.copy()
    for alpha in (0, 77, 128, 256):
        mix = (alpha * color.astype(np.int64) + (256 - alpha) * frames.astype(np.int64) + 128) >> 8
        want = np.where(depth[..., None] > 0, mix, frames)
        assert np.array_equal(_overlay(side, frames, color, depth, alpha), want.astype(np.uint8))
    with pytest.raises(_lib.BetaposeHipError, match=r"alpha must lie in 0 \.\. 256"):
        _overlay(side, frames, color, depth, 300)
    for a, k in zip((frames, color, depth), keep):                              # the read-only inputs were not written to
        assert np.array_equal(a, k) and not a.flags.writeable
