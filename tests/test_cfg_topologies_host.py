"""The cfg cases of tests/cfg_topologies.py on the host: each parses, its synthesized weight stream has the size the cfg
needs, the oracle (oracle/yolo_ref.py) runs it, rows and layers have the shapes the case states, and the values are finite
and O(1) -- so the relative bars tests/test_gpu_cfg_topologies.py holds the engine to mean something."""
import numpy as np
import pytest
import torch

import cfg_topologies as T
from betapose_amd import weights as W

NAMES = sorted(T.CASES)


def _trace(blocks, reso):
    """(C, H) per layer from the cfg alone (yolo/darknet.py:223-317 semantics), independent of the oracle's arithmetic."""
    out, c, h = [], 3, reso
    for i, b in enumerate(blocks):
        t = b["type"]
        if t == "convolutional":
            k, s = int(b["size"]), int(b["stride"])
            c, h = int(b["filters"]), (h + 2 * ((k - 1) // 2) - k) // s + 1
        elif t == "upsample":
            h *= int(b["stride"])
        elif t == "route":
            ls = [int(v) for v in b["layers"].split(",")]
            if len(ls) == 1:
                c, h = out[i + ls[0]]
            else:
                assert out[i + ls[0]][1] == out[ls[1]][1]
                c, h = out[i + ls[0]][0] + out[ls[1]][0], out[ls[1]][1]
        elif t == "shortcut":
            assert out[i - 1] == out[i + int(b["from"])]
        else:
            assert t == "yolo"
        out.append((c, h))
    return out


def test_the_case_table_is_complete():
    assert set(NAMES) == {"fallback_ops", "head_shared_96", "odd_channels_concat", "offset_mod4", "copy_concat_64", "heads_1", "heads_4",
                          "up_after_route", "shortcut_after_upsample", "fusable_trios",
                          "partial_s8_160", "partial_s8_96", "partial_s16_160", "partial_s16_96"}
    assert {n: T.reso(n) for n in NAMES if T.reso(n) != T.RESO} == {"partial_s8_160": 160, "partial_s8_96": 96, "partial_s16_160": 160, "partial_s16_96": 96}
    assert set(T.PARTIAL_CASES) == {n for n in NAMES if n.startswith("partial_")}
    assert set(T.SELECT_CASES) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_case_parses_and_its_stream_fits(name):
    blocks, expect = T.blocks(name), T.CASES[name][1]
    assert {b["type"] for b in blocks} <= {"convolutional", "shortcut", "upsample", "route", "yolo"}
    for b in blocks:
        if b["type"] == "convolutional":
            assert "pad" in b and b["activation"] in ("leaky", "linear")       # all the oracle knows
        if b["type"] == "upsample":
            assert b["stride"] == "2"
    yolos = [b for b in blocks if b["type"] == "yolo"]
    assert len(yolos) == expect["heads"] and all(int(b["classes"]) == expect["classes"] for b in yolos)
    assert len(blocks) - len(yolos) <= 16
    assert T.stream(name).size == W.darknet_stream_size(blocks)
    assert T.stream(name).dtype == np.float32 and bool(np.isfinite(T.stream(name)).all())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_runs_the_case(name):
    blocks, expect = T.blocks(name), T.CASES[name][1]
    x, rows, keep = T.oracle(name)
    assert x.shape == (2, 3, T.reso(name), T.reso(name)) and float(x.min()) >= 0.0 and float(x.max()) < 1.0
    assert rows.shape == (2, 3 * sum(g * g for g in expect["grids"]), 5 + expect["classes"])
    shapes = _trace(blocks, T.reso(name))
    assert sorted(keep) == list(range(len(blocks)))
    for i, (c, h) in enumerate(shapes):
        assert keep[i].shape == (2, c, h, h), (name, i)
    for i, ch in expect["shapes"].items():
        assert shapes[i] == ch, (name, i)
    heads = [shapes[i] for i, b in enumerate(blocks) if b["type"] == "yolo"]
    assert heads == [(3 * (5 + expect["classes"]), g) for g in expect["grids"]]
    assert bool(torch.isfinite(rows).all())
    for i, t in keep.items():
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) < 100.0, (name, i, float(t.abs().max()))
        assert float(t.abs().max()) > 1e-3, (name, i)                          # a dead layer would pass any relative bar
    # the two frames differ, and the oracle's batch of two is its two single frames (to fp32 re-association: the rows' fp32 bar)
    assert float((rows[0] - rows[1]).abs().max()) > 1e-4
    assert T.rows_close(rows[0], rows[1], "f32") is not None
    one = T.oracle(name, T.INPUT_SEED, 1)
    assert torch.equal(one[0][0], x[0]) and T.rows_close(one[1][0], rows[0], "f32") is None


@pytest.mark.parametrize("name", T.SELECT_CASES)
def test_select_cases_have_a_clear_arg_max(name):
    seed = T.select_seed(name)
    rows = T.oracle(name, seed)[1]
    assert float(T.objectness_margin(rows).min()) > 2 * T.PROB_TOL


def test_roots_follow_one_layer_routes_and_yolo_layers():
    assert T.roots("head_shared_96") == [0, 1, 2, 2, 2, 5, 6, 6]
    r = T.roots("heads_4")
    assert r[5] == 2 and r[11] == 8 and r[15] == 12 and r[19] == 18 and r[17] == 17
