"""``YoloNet`` on the cfgs of tests/cfg_topologies.py, in every precision, against the torch-CPU oracle of the same cfg
(oracle/yolo_ref.py; yolo/darknet.py:319-363 restated): the unfused add / upsample / channel-copy kernels and the plane
conversion behind them, concat views at odd offsets, concats of concats, a head tensor that is also a convolution's input, one
and four heads, and the fusion planner on groups it must and must not take.  None of this is planned for ``yolov3-single.cfg``.

Bars: the rows and per-layer bars tests/test_gpu_nets.py holds the default network to (restated in cfg_topologies.py with
pointers), plus identities between taps that hold bit for bit in every mode and so catch an index, stride or channel-offset
error a relative bar could absorb on a small tensor."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import cfg_topologies as T  # noqa: E402
from oracle import yolo_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(T.CASES)
_RUNS = {}


@pytest.fixture
def run(cuda, tmp_path_factory, request):
    """One engine per (case, precision), run once for all the tests on it (cfg_topologies.run_case); a failure to build or run it
    is every such test's failure."""
    name, precision = request.param
    key = (name, precision)
    if key not in _RUNS:
        try:
            net = T.make_net(name, tmp_path_factory.mktemp("cfg"), precision)
            _RUNS[key] = T.run_case(net, name)
        except Exception as e:       # (kept: the engine is not rebuilt and run again for each of the tests below)
            _RUNS[key] = e
    if isinstance(_RUNS[key], Exception):
        raise _RUNS[key]
    return name, precision, _RUNS[key]


every_run = pytest.mark.parametrize("run", [(n, p) for n in NAMES for p in T.PRECISIONS], indirect=True,
                                    ids=["%s-%s" % (n, p) for n in NAMES for p in T.PRECISIONS])


@every_run
def test_plan_is_what_the_case_claims(run):
    name, precision, r = run
    expect = T.CASES[name][1]
    bad = T.plan_misses(name, r["ops"], r["tiles"], precision in T.PLANE_MODES)
    assert not bad, "the case no longer tests what it is for: %s (%s, %s)" % (bad, r["ops"], r["tiles"])
    if precision not in T.PLANE_MODES:       # (f32, and bf16x3 on fp32 activations: no operand planes anywhere)
        assert not [c for c, t in r["tiles"].items() if t in T.PLANE_TILES]
    assert r["rows"] == 3 * sum(g * g for g in expect["grids"]) and r["attrs"] == 5 + expect["classes"]
    if expect["fuse"]:       # (below the planner's threshold of 48 blocks at batch 1 and 2: this run is the unfused kernels on 20-, 12-, 10- and 6-wide maps)
        assert r["fused_launches"] == [0, 0]
    # every layer that is not an alias, or a convolution living in its successor's epilogue, has a tap named by its index
    root = T.roots(name)
    assert set(r["taps"]) <= {str(i) for i in range(len(root)) if root[i] == i}
    assert {str(i) for i, b in enumerate(T.blocks(name)) if b["type"] == "route" and "," in b["layers"]} <= set(r["taps"])


@every_run
def test_rows_against_the_oracle(run):
    """Batch 1, and batch 2 on the engine built for 3: the heads' per-image strides with a short batch."""
    name, precision, r = run
    ref = T.oracle(name)[1]
    for b in range(2):
        assert r["rows1"][b].shape == ref[b].shape
        assert T.rows_close(r["rows1"][b], ref[b], precision) is None, (b, T.rows_close(r["rows1"][b], ref[b], precision))
    assert r["rows2"].shape == ref.shape
    assert T.rows_close(r["rows2"], ref, precision) is None, T.rows_close(r["rows2"], ref, precision)


@every_run
def test_taps_against_the_oracle(run):
    name, precision, r = run
    worst, bad = T.taps_vs_oracle(r["taps"], T.oracle(name)[2], precision)
    print("worst relative layer error %s %s %.2e" % (name, precision, worst))
    assert not bad, bad


@every_run
def test_exact_identities_between_taps(run):
    name, precision, r = run
    n, bad = T.identities(name, r["ops"], r["taps"])
    expect = T.CASES[name][1]
    concats = sum(1 for b in T.blocks(name) if b["type"] == "route" and "," in b["layers"])
    assert n == concats + sum(1 for op in set(expect["ops"]) if not op.startswith("concat"))
    assert not bad, bad


@every_run
def test_batch_of_two_equals_single_frames_and_repeats_bit_for_bit(run):
    name, precision, r = run
    for b in range(2):       # (K slices may differ with the batch size: the mode's bars, not bit equality)
        assert T.rows_close(r["rows2"][b], r["rows1"][b], precision) is None, (b, T.rows_close(r["rows2"][b], r["rows1"][b], precision))
    assert torch.equal(r["rows2"], r["rows2_again"])


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", T.SELECT_CASES)
def test_select_index_equals_the_oracles(cuda, tmp_path, name, precision):
    """``forward_select`` over one and four heads: the row index counts through the heads (YoloHead::row_off)."""
    seed = T.select_seed(name)
    x, ref, _ = T.oracle(name, seed)
    assert float(T.objectness_margin(ref).min()) > 2 * T.PROB_TOL          # precondition: a clear arg-max
    want = yolo_ref.select_index(ref, 0.01)
    assert (want >= 0).all()
    net = T.make_net(name, tmp_path, precision)
    sel, pred = net.forward_select(x.cuda(), confidence=0.01, num_classes=80, want_pred=True)
    assert T.rows_close(pred.cpu(), ref, precision) is None
    assert T.selected_index(sel).tolist() == want.tolist()
    assert T.selected_index(net.forward_select(x.cuda(), confidence=0.01, num_classes=80)).tolist() == want.tolist()   # decoded from the heads
    for b in range(2):
        assert T.selected_index(net.forward_select(x[b:b + 1].cuda(), confidence=0.01)).tolist() == [int(want[b])]


# ---- switches the engine reads once per process: a fresh child each
_CHILD_HEAD = r'''
import sys, tempfile, torch
sys.path.insert(0, "tests")
import cfg_topologies as T
tmp = tempfile.mkdtemp()
def check(name, precision, r):
    ref, keep = T.oracle(name)[1], T.oracle(name)[2]
    for b in range(2):
        assert T.rows_close(r["rows1"][b], ref[b], precision) is None, (name, precision, b, T.rows_close(r["rows1"][b], ref[b], precision))
    assert T.rows_close(r["rows2"], ref, precision) is None, (name, precision, T.rows_close(r["rows2"], ref, precision))
    worst, bad = T.taps_vs_oracle(r["taps"], keep, precision)
    print("worst relative layer error %s %s %.2e" % (name, precision, worst))
    assert not bad, (name, precision, bad)
    n, bad = T.identities(name, r["ops"], r["taps"])
    assert n > 0 and not bad, (name, precision, bad)
    assert torch.equal(r["rows2"], r["rows2_again"])
'''


def _child(code, env):
    r = subprocess.run([sys.executable, "-c", _CHILD_HEAD + code], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, **env))
    print(r.stdout[-3000:])
    return r


def test_bf16x3_on_the_operand_planes_runs_the_fallback_ops(cuda):
    """``BP_B3_PLANES=1``: the only way to the three-plane branch of f32_to_planes_kernel (conv_pl.hip), behind the unfused add /
    upsample / copy.  Same arithmetic as the default bf16x3 path, so the fp32 bars; the identities show the conversion left the
    fp32 tensors alone.  The convertible side of each conversion: ``shortcut_after_upsample`` (add), ``up_after_route`` (upsample),
    ``copy_concat_64`` (copy); ``odd_channels_concat`` is the side that cannot convert and stays on fp32."""
    code = r'''
for name in ("fallback_ops", "odd_channels_concat", "offset_mod4", "up_after_route", "shortcut_after_upsample", "copy_concat_64"):
    net = T.make_net(name, tmp, "bf16x3")
    r = T.run_case(net, name)
    bad = T.plan_misses(name, r["ops"], r["tiles"], True)      # (the convolutions behind the add / upsample / copy read the planes)
    assert not bad, (name, bad, r["tiles"])
    check(name, "bf16x3", r)
print("B3-PLANES-OK")
'''
    r = _child(code, {"BP_B3_PLANES": "1"})
    assert r.returncode == 0 and "B3-PLANES-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_fusion_takes_the_groups_it_may_and_equals_the_unfused_plan(cuda):
    """``BP_FUSE_MIN_BLOCKS=1`` lets the 16-patch groups of ``fusable_trios`` fuse.  The clean trio runs as one launch, the pair in
    front of the shortcut source as one launch, and the group whose first 1x1 is also a concat member as three: its output has a
    second reader.  Fused against ``set_fusion(False)`` at the bars of tests/test_gpu_fused.py (3e-5 of the layer's scale and the
    rows' fp32 bars in bf16x3; 1e-2 of the scale and the fp16 rows' bars in f16), and both against the oracle."""
    code = r'''
name = "fusable_trios"
for precision, rel in (("bf16x3", 3e-5), ("f16", 1e-2)):
    fused, plain = T.make_net(name, tmp, precision), T.make_net(name, tmp, precision)
    plain.set_fusion(False)
    assert plain.fused_launches(1) == 0
    tiles, IN_BLOCK, BLOCK = T.op_tiles(fused, 1), T.TILE_NONE, T.TILE_FUSED
    print(precision, "fused launches", fused.fused_launches(1), tiles)
    assert (tiles["conv1"], tiles["conv2"], tiles["conv3"]) == (IN_BLOCK, IN_BLOCK, BLOCK), "the clean trio is one launch"
    assert all(tiles["conv%d" % i] not in (IN_BLOCK, BLOCK) for i in (4, 5, 6)), "conv4's output is a concat member: it must be stored"
    assert (tiles["conv7"], tiles["conv8"]) == (IN_BLOCK, BLOCK) and tiles["conv9"] not in (IN_BLOCK, BLOCK), "conv8's output is a shortcut source"
    assert fused.fused_launches(1) == 2 and fused.fused_launches(2) == 2
    rf, rp = T.run_case(fused, name), T.run_case(plain, name)
    check(name, precision, rf)
    check(name, precision, rp)
    assert T.rows_close(rf["rows2"], rp["rows2"], precision) is None, T.rows_close(rf["rows2"], rp["rows2"], precision)
    for b in range(2):
        assert T.rows_close(rf["rows1"][b], rp["rows1"][b], precision) is None
    for k, t in rf["taps"].items():
        scale = max(1.0, float(rp["taps"][k].abs().max()))
        assert float((t - rp["taps"][k]).abs().max()) <= rel * scale, (precision, k, float((t - rp["taps"][k]).abs().max()), scale)
print("FUSION-OK")
'''
    r = _child(code, {"BP_FUSE_MIN_BLOCKS": "1"})
    assert r.returncode == 0 and "FUSION-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def _misses(r):
    """The child's "MISS" lines (cfg_topologies.fused_partial_case): which taps miss fused against unfused and at which pixels, the fused
    launches' own taps first."""
    return "\n".join(line for line in r.stdout.splitlines() if line.startswith("MISS"))[:6000] + "\n"


@pytest.mark.parametrize("name", T.PARTIAL_CASES)
def test_fused_blocks_on_partial_patches(cuda, name):
    """The fused block kernel (conv_fused.hip) on 20-, 12-, 10- and 6-wide maps, where patches hang over the right and the bottom edge: the
    halo's zeroing of intermediate pixels outside the image on interior patch positions, the pixel mask of the epilogue, ``TX = (W + 7) >> 3``.
    ``BP_FUSE_MIN_BLOCKS=1`` lets every group fuse at every batch size.  In bf16x3, f16 and f16r (cfg_topologies.fused_partial_case): the
    plan from ``op_tiles`` is the case's ``fuse`` table (a run that stayed unfused fails here); the fused engine and its ``set_fusion(False)``
    twin meet the oracle at the bars of every other case; fused against unfused at batch 1, 2 and 3 at the bars of tests/test_gpu_fused.py
    on the taps the fused launches themselves stored, with the pixel rows and columns that miss in the message.
    Forms: s8 <1,false,2> with the skip after the activation, <2,true,2> with CoutPad 128, <2,false,4> with two N tiles (bf16x3 only: fp16
    leaves it to the plane kernels); s16 <2,true,8> with a skip connection, <2,false,8> with Cout = 80 and the head refused as third member."""
    code = r'''
name = %r
for precision in ("bf16x3", "f16", "f16r"):
    T.fused_partial_case(name, tmp, precision, precision, check)
print("PARTIAL-OK")
''' % name
    r = _child(code, {"BP_FUSE_MIN_BLOCKS": "1"})
    assert r.returncode == 0 and "PARTIAL-OK" in r.stdout, _misses(r) + r.stdout[-2000:] + r.stderr[-3000:]


def test_fused_f16_pair_with_two_n_tiles_on_partial_patches(cuda):
    """``BP_FUSE_F16_ALL=1``: the fp16 <2,false,4> form (128 -> 64 -> 128, two N tiles per patch), compiled into every build and planned by
    none without the switch, on the 20-wide map; the same checks."""
    code = r'''
T.fused_partial_case("partial_s8_160", tmp, "f16", "f16+all", check)
print("F16-ALL-OK")
'''
    r = _child(code, {"BP_FUSE_MIN_BLOCKS": "1", "BP_FUSE_F16_ALL": "1"})
    assert r.returncode == 0 and "F16-ALL-OK" in r.stdout, _misses(r) + r.stdout[-2000:] + r.stderr[-3000:]
