"""Small detector cfgs that make ``YoloNet`` (betapose_amd/csrc/engine.cpp) plan what ``yolov3-single.cfg`` never does,
with the torch-CPU oracle (oracle/yolo_ref.py, yolo/darknet.py:319-363 restated) as the reference for every one of them.

The default cfg folds each [shortcut] and [upsample] into the epilogue of the convolution in front of it and makes every
route member a view into its concat buffer, so ``OP_ADD``, ``OP_UPSAMPLE``, ``OP_COPYCH`` (aux_kernels.hip add_kernel /
upsample2_kernel / copy_channels_kernel) and the plane conversion behind them (conv_pl.hip f32_to_planes_kernel) are
never launched by it.  The cases below emit them -- each of the three also with a plane-eligible convolution behind it, so
that the conversion runs (add: shortcut_after_upsample; upsample: up_after_route; copy: copy_concat_64) -- and the
topologies around them: a route of a route, a layer in two concats, view offsets of 2 mod 4 floats, 18- and 46-channel
concat members, a head tensor that is also a convolution's input, one head and four heads, and 1x1 -> 3x3 -> 1x1 groups
that the conv -> conv fusion (conv_fused.hip) may or may not take.

A case carries its resolution (``reso(name)``).  It is ``RESO`` = 64 unless the case says otherwise, the smallest the engine
takes: maps are 32, 16 or 8 wide.  The ``partial_*`` cases run at 160 and 96, where the maps behind strides 8 and 16 are 20, 10,
12 and 6 wide: no multiple of the fused block kernel's 8 x 8 output patch, which both default networks only ever run on maps
that are one.  Weights and inputs are seeded (betapose_amd/synth.py); nothing is read from a fixture.

Shared by tests/test_cfg_topologies_host.py (CPU) and tests/test_gpu_cfg_topologies.py (also from its child processes).
"""
import functools

import numpy as np
import torch

from betapose_amd import cfg as C, synth, weights as W
from oracle import yolo_ref

RESO = 64
WEIGHT_SEED, INPUT_SEED, DECOY_SEED = 7, 2024, 99
PRECISIONS = ("f32", "bf16x3", "f16", "f16r")
BOX_TOL, BOX_RTOL, PROB_TOL = 2e-3, 3e-5, 2e-5      # the fp32 bars of tests/test_gpu_nets.py (rows against the oracle)
LAYER_RTOL, LAYER_ATOL = 3e-5, 1e-5                 # ... test_yolo_layers_vs_oracle: |d| <= 3e-5 * scale + 1e-5
F16_CENTRE, F16_SIZE_ABS, F16_SIZE_REL, F16_PROB = 0.25, 5e-2, 2e-2, 5e-3     # ... _f16_rows_vs_oracle
F16_LAYER = 5e-2                                    # ... test_f16r_mode_fp16_skip_connections: |d| < 5e-2 * max(1, scale)
# kernel ids as Net::profile reports them (betapose_amd/csrc/bp_common.h, enum ConvTile): every tile that reads operand planes
# (conv_pl.hip conv_tile_is_pl: PL64, PL128, PL128x64, PL256x128, PLH128, S1, P3), the marker of a fused block's last member, and
# "launches nothing" (a member computed inside its block's launch)
PLANE_TILES = frozenset((13, 14, 15, 16, 25, 26, 27))
TILE_FUSED, TILE_NONE = 40, -1
PLANE_MODES = ("f16", "f16r")                       # the modes planned on operand planes (bf16x3 only under BP_B3_PLANES=1)


# ---------------------------------------------------------------- cfg text
def conv(filters, size=1, stride=1, act="leaky", bn=True):
    out = ["[convolutional]"]
    if bn:
        out.append("batch_normalize=1")
    out += ["filters=%d" % filters, "size=%d" % size, "stride=%d" % stride, "pad=1", "activation=%s" % act]
    return "\n".join(out) + "\n"


def head(classes):
    """The linear 1x1 convolution in front of a [yolo] layer."""
    return conv(3 * (5 + classes), 1, 1, "linear", bn=False)


def shortcut(frm):
    return "[shortcut]\nfrom=%d\nactivation=linear\n" % frm


def upsample():
    return "[upsample]\nstride=2\n"


def route(*layers):
    """One layer (relative): an alias.  Two layers (relative, absolute; yolo/darknet.py:347-352): a concat."""
    return "[route]\nlayers = %s\n" % ", ".join(str(v) for v in layers)


def yolo(classes, mask="0,1,2"):
    return "[yolo]\nmask = %s\nanchors = %s\nclasses=%d\nnum=9\n" % (mask, C.ANCHORS, classes)


def _cfg(*layers):
    return "\n".join(layers)


def _expect(ops, grids, classes=1, shapes=None, absent=(), planes=(), fp32=(), reso=RESO, fuse=None):
    """reso: the input resolution the case runs at; fuse: for the cases of the fused block kernel, what must run as one launch (FUSE_* below);
    ops: engine op names that must be in the plan; absent: op names that must NOT be (the layer is a view written in place, or
    lives in a convolution's epilogue); planes / fp32: convolutions that must / must not run on an operand-plane kernel in the plane
    modes; grids: the heads' grid sizes in cfg order; shapes: layer index -> (C, H) of the layers the case is about."""
    return {"ops": list(ops), "absent": list(absent), "planes": list(planes), "fp32": list(fp32), "heads": len(grids),
            "grids": list(grids), "classes": classes, "shapes": dict(shapes or {}), "reso": reso, "fuse": fuse}


# name -> (cfg text, expect).  The layer index is written in front of every line.
CASES = {
    # an unfused add (conv 2 is also routed), a shortcut of a shortcut onto itself, an unfused upsample, layers 5 and 0 in two
    # concats (the second one copies), a concat of concats (two more copies), an add reading a view with ld != C (layer 2
    # lives in concat 10)
    "fallback_ops": (_cfg(
        conv(20, 3, 2),         # 0   32x32
        conv(24, 3, 2),         # 1   16x16
        conv(24, 1, 1),         # 2
        shortcut(-2),           # 3   = 2 + 1
        shortcut(-1),           # 4   = 3 + 3
        upsample(),             # 5   32x32
        route(-1, 0),           # 6   [5, 0]   44 channels, views
        route(-2, 0),           # 7   [5, 0]   again: copies
        route(-1, 6),           # 8   [7, 6]   88 channels, copies
        conv(32, 3, 2),         # 9   16x16
        route(-1, 2),           # 10  [9, 2]   56 channels, views
        head(1),                # 11
        yolo(1),                # 12
    ), _expect(["shortcut3", "shortcut4", "upsample5", "concat7", "concat8"], [16],
               shapes={3: (24, 16), 5: (24, 32), 6: (44, 32), 7: (44, 32), 8: (88, 32), 10: (56, 16)})),
    # the first head's 96-channel tensor is also the input of a plane-eligible 1x1 convolution
    "head_shared_96": (_cfg(
        conv(32, 3, 2),         # 0   32x32
        conv(64, 3, 2),         # 1   16x16
        head(27),               # 2   96 channels
        yolo(27, "0,1,2"),      # 3
        route(-1),              # 4   = 2
        conv(64, 1, 1),         # 5
        head(27),               # 6
        yolo(27, "3,4,5"),      # 7
    ), _expect([], [16, 16], classes=27, shapes={2: (96, 16), 4: (96, 16), 6: (96, 16)}, planes=["conv5", "conv6"])),
    # 18 + 46 channels: first as views (the 18-channel convolution stores at an offset of 46 floats), then copied in the other
    # order into a second concat that a 3x3 convolution with Cin = 64 reads
    "odd_channels_concat": (_cfg(
        conv(32, 3, 2),         # 0   32x32
        conv(18, 1, 1),         # 1   A
        route(-2),              # 2   = 0
        conv(46, 1, 1),         # 3   B
        route(-1, 1),           # 4   [B, A]   views
        conv(32, 1, 1),         # 5
        route(-5, 3),           # 6   [A, B]   copies of 18 and 46 channels
        conv(64, 3, 1),         # 7
        route(-1, 5),           # 8   [7, 5]   96 channels, views
        conv(32, 3, 2),         # 9   16x16
        head(1),                # 10
        yolo(1),                # 11
    ), _expect(["concat6"], [16], shapes={4: (64, 32), 6: (64, 32), 8: (96, 32)}, absent=["concat4", "concat8"],
               planes=["conv5", "conv9"], fp32=["conv7"])),     # (conv 7 reads the copied 18 + 46 channels: that concat stays on fp32)
    # convolutions that store straight into a concat view 18 floats in: a plain one (layer 1) and one with the upsample in its
    # epilogue (layers 6 + 7)
    "offset_mod4": (_cfg(
        conv(32, 3, 2),         # 0   32x32
        conv(46, 1, 1),         # 1   B
        route(-2),              # 2   = 0
        conv(18, 1, 1),         # 3   A
        route(-1, 1),           # 4   [A, B]   B's view starts 18 floats in
        conv(64, 3, 2),         # 5   16x16
        conv(46, 1, 1),         # 6
        upsample(),             # 7   32x32, in conv 6's epilogue
        route(-6),              # 8   = 0
        conv(18, 1, 1),         # 9   A2
        route(-1, 7),           # 10  [A2, 7]  the upsampled store starts 18 floats in
        conv(32, 3, 2),         # 11  16x16
        route(-1, 5),           # 12  [11, 5]  96 channels
        head(1),                # 13
        yolo(1),                # 14
    ), _expect([], [16], shapes={4: (64, 32), 7: (46, 32), 10: (64, 32), 12: (96, 16)},
               absent=["concat4", "concat10", "concat12", "upsample7"], planes=["conv5", "conv11", "conv13"])),
    # 32 + 32 channels copied into a second concat that a 1x1 convolution with Cin = 64 reads on planes, and that 64-channel concat copied
    # 64 floats into a third one: the channel copy with the plane conversion behind it (offsets 0, 32 and 64; ld 64 and 128)
    "copy_concat_64": (_cfg(
        conv(32, 3, 2),         # 0   32x32
        conv(32, 1, 1),         # 1   A
        route(-2),              # 2   = 0
        conv(32, 3, 1),         # 3   B
        route(-1, 1),           # 4   [B, A]   views
        route(-4, 3),           # 5   [A, B]   copies of 32 channels each
        conv(64, 1, 1),         # 6
        route(-1, 4),           # 7   [6, 4]   128 channels: conv 6 a view, concat 4 copied 64 floats in
        conv(32, 3, 2),         # 8   16x16
        head(1),                # 9
        yolo(1),                # 10
    ), _expect(["concat5", "concat7"], [16], shapes={4: (64, 32), 5: (64, 32), 7: (128, 32)}, absent=["concat4"],
               planes=["conv6", "conv8", "conv9"])),
    "heads_1": (_cfg(
        conv(32, 3, 2),         # 0   32x32
        conv(32, 3, 2),         # 1   16x16
        conv(64, 3, 2),         # 2   8x8
        head(1),                # 3
        yolo(1, "6,7,8"),       # 4
    ), _expect([], [8])),
    "heads_4": (_cfg(
        conv(32, 3, 2),         # 0   32x32
        conv(32, 3, 2),         # 1   16x16
        conv(64, 3, 2),         # 2   8x8
        head(1),                # 3
        yolo(1, "6,7,8"),       # 4
        route(-3),              # 5   = 2
        conv(32, 1, 1),         # 6
        upsample(),             # 7   16x16, in conv 6's epilogue
        route(-1, 1),           # 8   [7, 1]
        head(1),                # 9
        yolo(1, "3,4,5"),       # 10
        route(-3),              # 11  = 8
        conv(32, 3, 1),         # 12
        head(1),                # 13
        yolo(1, "0,1,2"),       # 14
        route(-3),              # 15  = 12
        upsample(),             # 16  32x32, unfused (behind a route)
        route(-1, 0),           # 17  [16, 0]
        head(1),                # 18
        yolo(1, "1,2,3"),       # 19
    ), _expect(["upsample16"], [8, 16, 16, 32], shapes={8: (64, 16), 17: (64, 32)}, absent=["upsample7", "concat8", "concat17"],
               planes=["conv9", "conv12", "conv18"])),
    # an upsample behind a one-layer route and behind a concat; the second one's 64 channels go to a plane-eligible convolution
    "up_after_route": (_cfg(
        conv(32, 3, 2),         # 0   32x32
        conv(32, 3, 2),         # 1   16x16
        conv(32, 1, 1),         # 2
        route(-2),              # 3   = 1
        upsample(),             # 4   32x32
        route(-3, 1),           # 5   [2, 1]   16x16
        upsample(),             # 6   32x32, 64 channels
        conv(32, 1, 1),         # 7
        shortcut(-4),           # 8   = 7 + 4, in conv 7's epilogue
        head(1),                # 9
        yolo(1),                # 10
    ), _expect(["upsample4", "upsample6"], [32], shapes={4: (32, 32), 5: (64, 16), 6: (64, 32)}, absent=["concat5", "shortcut8"],
               planes=["conv7", "conv9"])),
    # a shortcut behind an upsample (its output a concat view that a plane-eligible convolution reads) and behind a route
    "shortcut_after_upsample": (_cfg(
        conv(32, 3, 2),         # 0   32x32
        conv(32, 3, 2),         # 1   16x16
        upsample(),             # 2   32x32, in conv 1's epilogue
        shortcut(-3),           # 3   = 2 + 0
        conv(32, 1, 1),         # 4
        route(-1, 3),           # 5   [4, 3]   views: the add stores into a view with ld 64
        route(-2),              # 6   = 4
        shortcut(-4),           # 7   = 4 + 3
        conv(32, 3, 2),         # 8   16x16
        head(1),                # 9
        yolo(1),                # 10
    ), _expect(["shortcut3", "shortcut7"], [16], shapes={3: (32, 32), 5: (64, 32), 7: (32, 32)}, absent=["upsample2", "concat5"],
               planes=["conv4", "conv8", "conv9"])),
    # three 1x1 -> 3x3 -> 1x1 groups at channel counts conv_fused_eligible() accepts (64 -> 64 -> 64): a clean one (1-3), one whose
    # first 1x1 is the second member of a later concat (4-6: its output has another reader and must be stored), one whose 3x3
    # output is a shortcut source (7-9: only the first two members can share a launch)
    "fusable_trios": (_cfg(
        conv(64, 3, 2),         # 0   32x32
        conv(64, 1, 1),         # 1
        conv(64, 3, 1),         # 2
        conv(64, 1, 1),         # 3
        conv(64, 1, 1),         # 4
        conv(64, 3, 1),         # 5
        conv(64, 1, 1),         # 6
        conv(64, 1, 1),         # 7
        conv(64, 3, 1),         # 8
        conv(64, 1, 1),         # 9
        shortcut(-2),           # 10  = 9 + 8, in conv 9's epilogue
        route(-1, 4),           # 11  [10, 4]  128 channels, views
        conv(32, 3, 2),         # 12  16x16
        head(1),                # 13
        yolo(1),                # 14
    ), _expect([], [16], shapes={10: (64, 32), 11: (128, 32)}, absent=["shortcut10", "concat11"],
               planes=["conv1", "conv2", "conv3", "conv5", "conv8", "conv12"])),
}

# ---- the fused block kernel (conv_fused.hip) on maps that are no multiple of its 8 x 8 patch.  Two cfgs (a case has at most 16 layers), each
# at 160 (maps 20 and 10 wide: full and partial patches in one launch, partial widths 4 and 2) and at 96 (12 wide: 4 patches, three of them
# partial; 6 wide: one patch, partial in both directions).  The template form <mid channels / 32, trailing 1x1, Cin / 32> stands behind each
# group.  At the default threshold of 48 blocks none of them fuses at batch 1 or 2; the tests that run them fused set BP_FUSE_MIN_BLOCKS=1.
# Each cfg holds one unfused shortcut of a layer onto itself: the identity between taps that every run is checked for.
_PARTIAL_S8 = _cfg(
    conv(32, 3, 2),         # 0
    conv(64, 3, 2),         # 1
    conv(64, 3, 2),         # 2   stride 8
    conv(32, 1, 1),         # 3
    conv(64, 3, 1),         # 4   pair 64 -> 32 -> 64                                  <1, false, 2>
    shortcut(-3),           # 5   = 4 + 2, in conv 4's epilogue (added after the activation)
    conv(64, 1, 1),         # 6
    conv(64, 3, 1),         # 7
    conv(128, 1, 1),        # 8   trio, CoutPad of the trailing 1x1 = 128               <2, true, 2>
    conv(64, 1, 1),         # 9
    conv(128, 3, 1),        # 10  pair 128 -> 64 -> 128: two N tiles per patch          <2, false, 4>
    shortcut(-3),           # 11  = 10 + 8, in conv 10's epilogue
    shortcut(-1),           # 12  = 11 + 11, unfused
    head(1),                # 13
    yolo(1),                # 14
)
_PARTIAL_S16 = _cfg(
    conv(32, 3, 2),         # 0
    conv(64, 3, 2),         # 1
    conv(64, 3, 2),         # 2
    conv(256, 3, 2),        # 3   stride 16
    conv(64, 1, 1),         # 4
    conv(64, 3, 1),         # 5
    conv(256, 1, 1),        # 6   the whole bottleneck shape                           <2, true, 8>
    shortcut(-4),           # 7   = 6 + 3, in conv 6's epilogue
    shortcut(-1),           # 8   = 7 + 7, unfused
    conv(64, 1, 1),         # 9
    conv(80, 3, 1),         # 10  pair 256 -> 64 -> 80: Cout no multiple of 64          <2, false, 8>
    head(1),                # 11  a 1x1 behind the pair, but from 80 channels: it cannot be the block's third member
    yolo(1),                # 12
)
# What runs as one launch under BP_FUSE_MIN_BLOCKS=1, by mode: the layer indices of each group's members.  bf16x3 takes every group.  The fp16 modes leave the 128 -> 64 -> 128 pair to the plane kernels (conv_fused.hip fused_form, the `g1 == 4` line) unless
# BP_FUSE_F16_ALL is set ("f16+all").
FUSE_S8 = {"bf16x3": [(3, 4), (6, 7, 8), (9, 10)], "f16": [(3, 4), (6, 7, 8)], "f16r": [(3, 4), (6, 7, 8)],
           "f16+all": [(3, 4), (6, 7, 8), (9, 10)]}
FUSE_S16 = {"bf16x3": [(4, 5, 6), (9, 10)], "f16": [(4, 5, 6), (9, 10)], "f16r": [(4, 5, 6), (9, 10)]}
for _r in (160, 96):
    CASES["partial_s8_%d" % _r] = (_PARTIAL_S8, _expect(
        ["shortcut12"], [_r // 8], shapes={2: (64, _r // 8), 5: (64, _r // 8), 8: (128, _r // 8), 11: (128, _r // 8), 12: (128, _r // 8)},
        absent=["shortcut5", "shortcut11"], reso=_r, fuse=FUSE_S8))
    CASES["partial_s16_%d" % _r] = (_PARTIAL_S16, _expect(
        ["shortcut8"], [_r // 16], shapes={3: (256, _r // 16), 7: (256, _r // 16), 8: (256, _r // 16), 10: (80, _r // 16)},
        absent=["shortcut7"], reso=_r, fuse=FUSE_S16))
PARTIAL_CASES = tuple(sorted(n for n in CASES if CASES[n][1]["fuse"]))
SELECT_CASES = ("heads_1", "heads_4")


# ---------------------------------------------------------------- weights, inputs, oracle
@functools.lru_cache(None)
def blocks(name):
    return C.parse_cfg_text(CASES[name][0])


@functools.lru_cache(None)
def stream(name):
    return synth.synth_yolo_stream(WEIGHT_SEED, blocks(name))


def reso(name):
    return CASES[name][1]["reso"]


def rand_input(seed, batch=2, reso=RESO):
    return torch.rand(batch, 3, reso, reso, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(None)
def oracle(name, seed=INPUT_SEED, batch=2):
    """(input [batch,3,reso,reso], oracle rows [batch, rows, attrs], {layer index: NCHW output}) -- computed once per case and
    shared; callers must not write to them."""
    x = rand_input(seed, batch, reso(name))
    keep = {}
    rows = yolo_ref.darknet_forward(blocks(name), W.split_darknet_stream(blocks(name), stream(name)), x, reso=reso(name), keep=keep)
    return x, rows, keep


def objectness_margin(rows):
    """Per image: best minus second-best objectness."""
    top = torch.topk(rows[:, :, 4], 2, dim=1).values
    return top[:, 0] - top[:, 1]


@functools.lru_cache(None)
def select_seed(name):
    """The first input seed (from INPUT_SEED) at which the oracle's best and second-best objectness of every image differ by
    more than 2 * PROB_TOL: an engine within PROB_TOL of the oracle must then select the same row."""
    for seed in range(INPUT_SEED, INPUT_SEED + 20):
        if float(objectness_margin(oracle(name, seed)[1]).min()) > 2 * PROB_TOL:
            return seed
    raise AssertionError("no input seed with a clear objectness arg-max for " + name)


def roots(name):
    """Layer index -> the layer whose tensor (and tap) holds its output: a one-layer route and a [yolo] layer are aliases."""
    out = []
    for i, b in enumerate(blocks(name)):
        r = i
        if b["type"] == "route":
            ls = [int(v) for v in b["layers"].split(",")]
            if len(ls) == 1:
                r = out[i + ls[0]]
        elif b["type"] == "yolo":
            r = out[i - 1]
        out.append(r)
    return out


# ---------------------------------------------------------------- engine runs and the checks on them
def write_cfg(name, directory):
    path = str(directory) + "/%s.cfg" % name
    with open(path, "w") as f:
        f.write(CASES[name][0])
    return path


def make_net(name, directory, precision, max_batch=3):
    from betapose_amd.darknet import Darknet
    net = Darknet(write_cfg(name, directory), reso=reso(name), max_batch=max_batch).load_stream(stream(name)).cuda().eval()
    net.set_precision(precision)
    return net


def run_case(net, name, seed=INPUT_SEED):
    """One engine through the case's inputs.  A full batch of other frames goes first, so that a tensor the plan forgets to
    store holds another input's values, not this one's from an earlier call.  The taps are read last layer first: reading a
    tap may rebuild its tensor (Net::tap_copy), which must not repair what a later layer has already read."""
    x = oracle(name, seed)[0].cuda()
    net(rand_input(DECOY_SEED, net.max_batch, reso(name)).cuda())
    out = {"ops": [n for n, _ in net.op_names()], "rows": net.rows, "attrs": net.attrs}
    out["rows1"] = [net(x[b:b + 1]).cpu()[0] for b in range(x.shape[0])]
    out["rows2"] = net(x).cpu()
    out["rows2_again"] = net(x).cpu()
    taps = net.taps()
    out["taps"] = {}
    for i in reversed(range(len(taps))):
        out["taps"][taps[i][0]] = net.tap(i, batch=x.shape[0]).cpu()
    out["tiles"] = op_tiles(net, x.shape[0])
    out["fused_launches"] = [net.fused_launches(b) for b in (1, 2)]
    return out


def op_tiles(net, batch):
    """Op name up to its first blank ("conv4 k1 32x32 64->64 s1" -> "conv4") -> the kernel id Net::profile reports for it at this batch
    size.  (Several copies of one concat share a name; they are not convolutions and their id is not looked at.)"""
    info = net.profile(batch, 1)[1]
    return {n.split()[0]: int(info[i, 1]) for i, (n, _) in enumerate(net.op_names())}


def plan_misses(name, ops, tiles, on_planes):
    """What of the case's stated plan does not hold: ops that must be / must not be in it and, when the engine is in a mode planned on
    operand planes, the convolutions that must / must not read them."""
    expect, bad = CASES[name][1], []
    bad += ["%s is not in the plan" % op for op in expect["ops"] if op not in ops]
    bad += ["%s is in the plan" % op for op in expect["absent"] if op in ops]
    if on_planes:
        bad += ["%s is not on a plane kernel (tile %d)" % (c, tiles[c]) for c in expect["planes"] if tiles[c] not in PLANE_TILES]
        bad += ["%s is on a plane kernel (tile %d)" % (c, tiles[c]) for c in expect["fp32"] if tiles[c] in PLANE_TILES]
    return bad


def rows_close(got, ref, precision):
    """None when ``got`` meets the mode's bars against ``ref`` ([..., rows, attrs]), else what misses."""
    d = (got - ref).abs()
    if not bool(torch.isfinite(got).all()):
        return "non-finite rows"
    if precision in ("f32", "bf16x3"):
        if not bool((d[..., :4] <= BOX_TOL + BOX_RTOL * ref[..., :4].abs()).all()):
            return "boxes: max |d| %.3e" % float(d[..., :4].max())
        if float(d[..., 4:].max()) > PROB_TOL:
            return "probabilities: max |d| %.3e" % float(d[..., 4:].max())
        return None
    if not float(d[..., :2].max()) < F16_CENTRE:
        return "centres: max |d| %.3e px" % float(d[..., :2].max())
    if not bool((d[..., 2:4] <= F16_SIZE_ABS + F16_SIZE_REL * ref[..., 2:4].abs()).all()):
        return "sizes: max |d| %.3e" % float(d[..., 2:4].max())
    if not float(d[..., 4:].max()) < F16_PROB:
        return "probabilities: max |d| %.3e" % float(d[..., 4:].max())
    return None


def taps_vs_oracle(taps, keep, precision):
    """(worst relative error, [what misses the mode's per-layer bar])."""
    worst, bad = 0.0, []
    for tap_name, got in taps.items():
        ref = keep[int(tap_name)]
        if got.shape != ref.shape:
            bad.append("layer %s: shape %s, oracle %s" % (tap_name, tuple(got.shape), tuple(ref.shape)))
            continue
        d = float((got - ref).abs().max())
        scale = float(ref.abs().max()) + 1e-6
        worst = max(worst, d / scale)
        ok = d <= LAYER_RTOL * scale + LAYER_ATOL if precision in ("f32", "bf16x3") else d < F16_LAYER * max(1.0, scale)
        if not (ok and bool(torch.isfinite(got).all())):
            bad.append("layer %s: max |d| %.3e (scale %.2f)" % (tap_name, d, scale))
    return worst, bad


def identities(name, ops, taps):
    """The relations between taps that hold bit for bit in every mode, whatever the convolutions computed: an unfused
    upsample is the nearest-neighbour copy of its source, a concat is its members side by side, an unfused shortcut is the
    fp32 sum of its two inputs.  Returns (number checked, [what does not hold])."""
    root, bl = roots(name), blocks(name)
    n, bad = 0, []
    for i, b in enumerate(bl):
        if str(i) not in taps:
            continue
        t = b["type"]
        if t == "upsample" and "upsample%d" % i in ops:
            want = taps[str(root[i - 1])].repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        elif t == "route" and "," in b["layers"]:
            ls = [int(v) for v in b["layers"].split(",")]
            want = torch.cat((taps[str(root[i + ls[0]])], taps[str(root[ls[1]])]), 1)
        elif t == "shortcut" and "shortcut%d" % i in ops:
            want = taps[str(root[i - 1])] + taps[str(root[i + int(b["from"])])]
        else:
            continue
        n += 1
        if not torch.equal(taps[str(i)], want):
            bad.append("%s %d: max |d| %.3e" % (t, i, float((taps[str(i)] - want).abs().max())))
    return n, bad


# ---------------------------------------------------------------- the fused block kernel on partial patches (PARTIAL_CASES)
FUSED_REL = {"bf16x3": 3e-5, "f16": 1e-2, "f16r": 1e-2}     # tests/test_gpu_fused.py, fused against unfused: |d| <= rel * max(1, scale)


def fuse_plan_misses(name, key, tiles, launches):
    """What of the case's fusion plan ``CASES[name][1]["fuse"][key]`` does not hold in ``tiles`` (op_tiles) and the engine's count of
    fused launches: a group that is to fuse reports TILE_NONE for every member but the last and TILE_FUSED for that one; no other
    convolution reports either -- a group that stays unfused, and the head behind the 80-channel pair, which cannot be a third member."""
    expect, bad = CASES[name][1]["fuse"][key], []
    for g in expect:
        got, want = tuple(tiles["conv%d" % i] for i in g), (TILE_NONE,) * (len(g) - 1) + (TILE_FUSED,)
        if got != want:
            bad.append("group %s reports tiles %s, not one fused launch %s" % (g, got, want))
    members = {i for g in expect for i in g}
    bad += ["%s is not in a group that may fuse but reports tile %d" % (c, t) for c, t in sorted(tiles.items())
            if c.startswith("conv") and int(c[4:]) not in members and t in (TILE_NONE, TILE_FUSED)]
    if launches != len(expect):
        bad.append("%d fused launches, not %d" % (launches, len(expect)))
    return bad


def evidence_taps(name, tiles, tap_names):
    """The taps a fused launch stored: those of the convolutions that report TILE_FUSED (named by the shortcut behind the convolution where
    that lives in its epilogue).  A tensor that exists only inside a block is rebuilt for its tap by the unfused launches (Net::tap_copy):
    it says nothing about the fused kernel."""
    bl, out = blocks(name), []
    for c, t in tiles.items():
        if c.startswith("conv") and t == TILE_FUSED:
            i = int(c[4:])
            folded = bl[i + 1]["type"] == "shortcut" and str(i) not in tap_names
            out.append(str(i + 1) if folded else str(i))
    return sorted(out, key=int)


def where_off(d, bar):
    """Where |d| ([batch, C, H, W]) is over ``bar`` on a map cut into 8 x 8 patches from its top left corner.  Per region -- the pixels of
    full patches, the columns of the partial patches at the right edge, the rows of those at the bottom edge -- the maximum and how many pixels
    are over the bar; then the pixel columns over the bar above the bottom strip and the pixel rows over the bar left of the right strip (a
    mask wrong by one pixel shows as a single column or row there)."""
    px = torch.nan_to_num(d, nan=float("inf")).amax(dim=(0, 1))
    hf, wf = 8 * (px.shape[0] // 8), 8 * (px.shape[1] // 8)
    over = px > bar
    yl, xl = hf or px.shape[0], wf or px.shape[1]      # (a map of one partial patch: every row, every column)

    def region(what, t, o):
        return "%s max %.3e, %d of %d pixels over the bar" % (what, float(t.max()) if t.numel() else 0.0, int(o.sum()), o.numel())
    return "; ".join((region("full-patch pixels (y < %d, x < %d)" % (hf, wf), px[:hf, :wf], over[:hf, :wf]),
                      region("partial column strip (x >= %d)" % wf, px[:, wf:], over[:, wf:]),
                      region("partial row strip (y >= %d)" % hf, px[hf:, :], over[hf:, :]),
                      "columns over the bar at y < %d: %s" % (yl, torch.nonzero(over[:yl].any(0)).flatten().tolist()),
                      "rows over the bar at x < %d: %s" % (xl, torch.nonzero(over[:, :xl].any(1)).flatten().tolist())))


def run_batch(net, x):
    """(rows, {tap name: NCHW tensor}) of one call; the taps are read last layer first (see run_case)."""
    rows = net(x.cuda()).cpu()
    names = net.taps()
    return rows, {names[i][0]: net.tap(i, batch=x.shape[0]).cpu() for i in reversed(range(len(names)))}


def fused_vs_plain(precision, rf, rp, picked):
    """``rf``, ``rp``: run_batch of the fused engine and of its set_fusion(False) twin on one input.  Rows at the mode's bars, every tap at
    FUSED_REL of its scale.  -> (worst |d| / max(1, scale) over the ``picked`` taps, [what misses]); a picked tap that was not compared
    is a miss."""
    worst, first, bad, rel = 0.0, [], [], FUSED_REL[precision]
    if rows_close(rf[0], rp[0], precision) is not None:
        bad.append("rows: " + rows_close(rf[0], rp[0], precision))
    compared = set()
    for k, t in rf[1].items():
        ref = rp[1][k]
        d, scale = (t - ref).abs(), max(1.0, float(ref.abs().max()))
        if k in picked:
            compared.add(k)
            worst = max(worst, float(d.max()) / scale)
        if not (float(d.max()) <= rel * scale and bool(torch.isfinite(t).all())):
            (bad if k not in picked else first).append("layer %s%s: max |d| %.3e over %.3e (scale %.2f): %s" % (k, " (stored by a fused launch)" if k in picked else "", float(d.max()), rel * scale, scale, where_off(d, rel * scale)))
    first += ["tap %s was stored by a fused launch and was not compared" % k for k in picked if k not in compared]
    return worst, first[::-1] + bad         # (the fused launches' own taps first, in layer order)


def fused_partial_case(name, directory, precision, key, check):
    """One PARTIAL_CASES case in one mode under BP_FUSE_MIN_BLOCKS=1 (set by the caller's process): the plan is the case's
    ``fuse[key]`` at batch 1, 2 and 3; fused against unfused at batch 1 (either image), 2 and 3 (the oracle holds two images: the third is
    another seed's) with the taps the fused launches stored named first in a miss; then the fused engine and its unfused twin both meet
    ``check`` (the oracle's rows and layers, the identities, the repeat)."""
    fused, plain = make_net(name, directory, precision), make_net(name, directory, precision)
    plain.set_fusion(False)
    picked = None
    for b in (1, 2, 3):
        assert plain.fused_launches(b) == 0
        tiles = op_tiles(fused, b)
        bad = fuse_plan_misses(name, key, tiles, fused.fused_launches(b))
        assert not bad, (name, key, b, bad, tiles)
        taps = evidence_taps(name, tiles, [t[0] for t in fused.taps()])
        assert picked in (None, taps) and len(taps) == len(CASES[name][1]["fuse"][key])
        picked = taps
    # fused against unfused first: both plans read the same input, so a wrong border pixel is not diluted by the layers in front, and the
    # message says where it is
    x = oracle(name)[0]
    x3 = torch.cat((x, rand_input(INPUT_SEED + 1, 1, reso(name))))
    fused(rand_input(DECOY_SEED, fused.max_batch, reso(name)).cuda())
    for b, xb in ((1, x[:1]), (1, x[1:]), (2, x), (3, x3)):
        worst, bad = fused_vs_plain(precision, run_batch(fused, xb), run_batch(plain, xb), picked)
        print("fused against unfused %s %s batch %d taps %s: worst |d| / max(1, scale) %.2e" % (name, key, b, ",".join(picked), worst))
        for m in bad:
            print("MISS %s %s batch %d: %s" % (name, key, b, m))
        assert not bad, (name, key, b, bad[0])
    rf, rp = run_case(fused, name), run_case(plain, name)
    assert set(picked) <= set(rf["taps"]), (picked, sorted(rf["taps"]))       # (check compares every tap of the run with the oracle's layer)
    check(name, precision, rf)
    check(name, precision, rp)


def selected_index(sel):
    return sel[:, 0].contiguous().cpu().view(torch.int32).numpy().astype(np.int64)
