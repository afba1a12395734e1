"""The training iteration's host twins (betapose_amd/darknet_train.py with device=None, csrc/darknet_train_host.cpp)
against the reference's own C code recorded in tests/golden/darknet_train.npz (tools/make_golden_darknet_train.py).  A
quantity's bar is max(4 * ref_err, 2^-23) with ref_err the reference's own distance from a float64 evaluation, read
from the archive.  No GPU needed."""
import os

import numpy as np
import pytest

import darknet_train_common as D
from betapose_amd import _lib, weights as W
from betapose_amd.darknet_train import TrainableDarknet, learning_rate, net_options
from betapose_amd import cfg as C


@pytest.mark.parametrize("name", ["a0", "a1"])
def test_one_step_against_the_reference(name):
    """group A: every convolution's output, batch mean and variance, every update buffer before the update, every
    parameter, rolling statistic and update buffer after it, the cost; the yolo deltas' non-zero sets are equal."""
    g = D.golden()
    quantities, deltas = D.group_a_step(D.make_net(name), name)
    for h, d in enumerate(deltas):
        ref = g["%s.0.yolo%d.delta" % (name, h)]
        assert np.array_equal(d != 0, ref != 0), "head %d: the non-zero deltas differ in place" % h
    assert len(quantities) > 60
    for q, v in quantities.items():
        D.check(q, v)


def test_subdivisions_two_updates_in_four_calls():
    """group B: the state after each call; calls 1 and 3 leave the parameters alone; the rate of each call"""
    g = D.golden()
    net = D.make_net("b")
    for k in range(4):
        before = net.state()
        inps, truth = D.case_batch("b", k)
        cost = net.train_step(inps, truth)
        D.check("b.%d.cost" % k, np.float32(cost))
        after = net.state()
        for q, v in after.items():
            D.check("b.%d.post.%s" % (k, q), v)
        params = [q for q in after if q.split(".")[1] in ("weights", "biases", "scales")]
        same = all(np.array_equal(before[q], after[q]) for q in params)
        assert same == (k in (0, 2)), "an update belongs after calls 2 and 4 only"
        assert np.float32(net.current_rate()) == g["b.%d.rate" % k]


def test_learning_rate_policies():
    """get_current_rate across burn_in and every policy, to one float32 ulp"""
    g, m = D.golden(), D.meta()["rates"]
    assert set(m) == {"constant", "steps", "step", "exp", "poly"}
    for pol, c in m.items():
        net = net_options(C.parse_cfg_text(c["cfg"])[0])
        for b, ref in zip(c["batches"], g["rates." + pol]):
            ours = learning_rate(net, b)
            assert abs(float(ours) - float(ref)) <= float(np.spacing(np.float32(ref))), (pol, b, ours, ref)


@pytest.fixture(scope="module")
def short_run():
    net = D.make_net("c")
    inps, truth = D.case_batch("c", 0)
    return net, [net.train_step(inps, truth) for _ in range(D.meta()["cases"]["c"]["calls"])]


def test_short_run_costs_and_final_parameters(short_run):
    """group C: 20 calls on one batch: the cost sequence and the final parameters within their bars, the cost falling"""
    net, costs = short_run
    D.check("c.costs", np.array(costs, np.float32))
    assert costs[-1] < costs[0]
    for q, v in net.state().items():
        D.check("c.19.post.%s" % q, v)


def test_save_weights_gives_the_reference_file(tmp_path, short_run):
    """fed the reference's final parameters, save_weights gives the reference's file byte for byte; a file written after
    our own run reads back through weights.py to state(), and loads into a new net"""
    ref_file = bytes(D.golden()["c.weights_file"])
    net = D.make_net("c")
    net.load_state(D.state_of("c", 19))
    net.seen = 20 * net.net["batch"]
    p = str(tmp_path / "ref.weights")
    net.save_weights(p)
    assert open(p, "rb").read() == ref_file
    ours, _ = short_run
    p = str(tmp_path / "ours.weights")
    ours.save_weights(p)
    _, seen, flat = W.read_darknet_weights(p)
    assert seen == ours.seen == 60
    st = ours.state()
    for n, part in enumerate(W.split_darknet_stream(ours.blocks[1:], flat)):
        assert np.array_equal(part["weight"], st["conv%d.weights" % n])
        assert np.array_equal(part["bn_bias"] if part["bn"] else part["bias"], st["conv%d.biases" % n])
        if part["bn"]:
            assert np.array_equal(part["bn_weight"], st["conv%d.scales" % n])
            assert np.array_equal(part["bn_mean"], st["conv%d.rolling_mean" % n])
            assert np.array_equal(part["bn_var"], st["conv%d.rolling_variance" % n])
    again = TrainableDarknet(D.meta()["cases"]["c"]["cfg"], weights=p)
    assert again.seen == 60 and TrainableDarknet(D.meta()["cases"]["c"]["cfg"], weights=p, clear=True).seen == 0
    assert all(np.array_equal(v, again.state()[q]) for q, v in st.items() if not q.endswith("_updates"))


BASE = D.meta()["cases"]["a0"]["cfg"]


@pytest.mark.parametrize("old, new, key", [
    ("random=0", "random=1", "random"), ("momentum=0.9", "momentum=0.9\nadam=1", "adam"),
    ("activation=leaky", "activation=leaky\nstopbackward=1", "stopbackward"), ("random=0", "random=0\nfocal_loss=1", "focal_loss"),
    ("activation=leaky", "activation=leaky\nxnor=1", "xnor"), ("activation=leaky", "activation=mish", "activation"),
    ("size=3", "size=5", "size"), ("stride=2\npad", "stride=3\npad", "stride"), ("[upsample]\nstride=2", "[upsample]\nstride=4", "stride"),
    ("[upsample]\nstride=2", "[maxpool]\nsize=2\nstride=2", "maxpool"), ("policy=steps", "policy=sigmoid", "policy"),
    ("from=-3\nactivation=linear", "from=-3\nactivation=leaky", "activation"), ("layers = -1, 0", "layers = -1, 0, 0", "layers"),
    ("pad=1", "pad=0", "pad")])
def test_unsupported_keys_raise_with_their_name(old, new, key):
    assert old in BASE
    with pytest.raises(ValueError, match="'%s'" % key):
        TrainableDarknet(BASE.replace(old, new, 1))


def test_update_twin_equals_three_numpy_passes():
    rows = D.update_case()
    a, dk, mom = np.float32(0.01) / np.float32(6), np.float32(-0.0005) * np.float32(6), np.float32(0.9)
    ref = D.update_reference(rows, a, dk, mom)
    mine = [(p.copy(), u.copy(), k) for p, u, k in rows]
    table = np.array([(p.ctypes.data, u.ctypes.data, p.size, k) for p, u, k in mine], np.int64)
    _lib.check(_lib.lib().bp_train_update_host(table.ctypes.data, len(mine), float(a), float(dk), float(mom)))
    for (p, u, _), (rp, ru) in zip(mine, ref):
        assert np.array_equal(p.view(np.uint32), rp.view(np.uint32)) and np.array_equal(u.view(np.uint32), ru.view(np.uint32))


@pytest.mark.parametrize("shape", D.CONV_SHAPES, ids=[s[0] for s in D.CONV_SHAPES])
def test_host_gemm_roles_within_the_chain_bound(shape):
    """each role's host twin against float64: an fmaf chain of K terms is within (K + 2) 2^-24 sum|a b| of the exact sum"""
    x, w, dy, dx0, wu0 = D.conv_case(shape)
    stride = shape[7]
    for role in (0, 1, 2):
        xs, ws, ys = (dx0.copy() if role == 2 else x.copy()), (wu0.copy() if role == 1 else w.copy()), dy.copy()
        if role == 0:
            ys[...] = np.nan
        D.run_conv(role, shape, xs, ws, ys)
        ours = (ys, ws, xs)[role]
        exact = D.conv_reference(role, x, w, dy, dx0, wu0, stride)
        mag = D.conv_reference(role, np.abs(x), np.abs(w), np.abs(dy), np.abs(dx0), np.abs(wu0), stride)
        terms = {0: w[0].size, 1: dy.size // dy.shape[1], 2: w.shape[0] * w.shape[2] ** 2}[role]
        assert np.all(np.abs(ours - exact) <= (terms + 4) * 2.0 ** -24 * mag + 1e-30), (shape[0], role)
        # what the role does not write stays as it was
        assert np.array_equal(ys, dy) or role == 0
        assert np.array_equal(ws, w) or role == 1
        assert np.array_equal(xs, x) or role == 2


@pytest.mark.parametrize("N, C, S", D.BN_SHAPES)
def test_host_batch_norm_against_float64(N, C, S):
    """mean and variance (N * S - 1) and x_norm against numpy float64; the linear, bias-only form"""
    c = D.bn_case(N, C, S)
    r = D.run_bn(c, N, C, S, 1, 1)
    x = c["x"].astype(np.float64)
    mean = x.mean((0, 2))
    var = ((x - mean[None, :, None]) ** 2).sum((0, 2)) / (N * S - 1)
    assert np.abs(r["mean"] - mean).max() <= 2e-7 * np.abs(x).max()
    assert np.abs(r["var"] - var).max() <= 4e-7 * var.max()
    xn = (x - mean[None, :, None]) / (np.sqrt(var) + 1e-6)[None, :, None]
    assert np.abs(r["x_norm"] - xn).max() <= 2e-6 * np.abs(xn).max()
    assert np.allclose(r["rolling_mean"], .9 * c["rolling_mean"] + .1 * mean, rtol=0, atol=1e-6)
    lin = D.run_bn(c, N, C, S, 0, 0)
    assert np.array_equal(lin["out"], c["x"] + c["biases"][None, :, None]) and np.array_equal(lin["delta"], c["delta"])
    assert np.allclose(lin["bias_updates"], c["bias_updates"] + c["delta"].astype(np.float64).sum((0, 2)), rtol=0, atol=1e-5)


def test_batch_of_one_value_is_an_argument_error():
    c = D.bn_case(1, 4, 1)
    with pytest.raises(_lib.BetaposeHipError, match="batch \\* spatial"):
        D.run_bn(c, 1, 4, 1, 1, 1)


def test_the_library_still_exports_what_the_header_declares():
    import helpers
    assert {"bp_train_conv", "bp_train_conv_host", "bp_train_bn_forward", "bp_train_bn_backward", "bp_train_update",
            "bp_train_update_host"} <= helpers.header_names() == set(_lib.PROTOTYPES)
