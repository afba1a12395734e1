"""The training iteration's host twins (betapose_amd/darknet_train.py with device=None, csrc/darknet_train_host.cpp)
against the reference's own C code recorded in tests/golden/darknet_train.npz (tools/make_golden_darknet_train.py).  A
quantity's bar is max(4 * ref_err, 2^-23) with ref_err the reference's own distance from a float64 evaluation, read
from the archive.  The shipped topology's step has an archive of its own, tests/golden/darknet_train_shipped.npz, which
holds the bars only: there the float64 step of tests/darknet_train_f64.py is the other side.  No GPU needed."""
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


def test_shipped_topology_one_step_within_the_reference_bars():
    """One step of cfg.yolov3_single_cfg_text(1) (random=0) on a 64 x 32 input, batch 2 -- 75 convolutions up to 1024
    channels, chains of 4608 and 9216 terms, routes to layers 36 and 61, batch norms over 4 values -- on the host twin,
    the reference's yolo deltas going in, against the float64 step teacher-forced on the twin's own leaky masks.  Every
    bar is max(4 ref_err, 2^-23) of tests/golden/darknet_train_shipped.npz: the reference's own distance from the
    float64 step teacher-forced on ITS masks.  At most 1 in 10 000 leaky outputs may differ in sign from the free
    float64 forward (the maker held the reference to a quarter of that)."""
    g = D.golden(D.SHIPPED)
    q, deltas, _, info = D.shipped_host()
    print("the host twin's step: %.1f s" % info["seconds"])
    for h, d in enumerate(deltas):
        ref = g["shipped.0.yolo%d.delta" % h]
        assert np.array_equal(d != 0, ref != 0), "head %d: the non-zero deltas differ in place" % h
    sizes = [v.size for k, v in q.items() if k.startswith("shipped.0.post.") and k.split(".")[-1] in ("weights", "biases", "scales")]
    chunk = int(_lib.lib().bp_train_update_chunk())
    assert info["rows"] == len(sizes) == 222
    assert info["blocks"] == sum((n + chunk - 1) // chunk for n in sizes)
    D.check_shipped(q, "host twin")


def test_non_square_tiny_net_against_float64():
    """case a0's net on a 24 x 16 input: one train_step on the host twin against the free-running float64 step on the
    same seeded batch, under a0's bars for the same quantity names (the layer set and depth are a0's).  The batch obeys
    the fixture maker's conditions, so no leaky mask and no assignment of the heads can differ between the two."""
    text, st, x, t = D.tiny_wide()
    net, _, convs, heads = D.parsed(text)
    q, _ = D.tiny_wide_step()
    ok, gaps = D.conditions({k[len("a0.0."):]: v for k, v in q.items()}, convs, heads, t, net)
    assert ok, gaps
    exact, _ = D.f64_quantities(text, st, x, "a0", truth=t, blas=False)
    assert set(exact) - set(q) == {k for k in exact if ".pre." in k} and len(exact) > 60
    for k, v in exact.items():
        if ".pre." not in k:
            D.check(k, q[k], against=v)


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
    """mean and variance (N * S - 1) and x_norm against numpy float64; the linear, bias-only form.

    x_norm at a count of 2: the two values of a channel may lie much closer to each other than to 0, and x - mean then
    inherits the float32 mean's rounding, u |mean| with u = 2^-24, whatever the difference is; no bound relative to
    max|x_norm| holds over 1024 such channels.  There the bound is per element, from the operations: the mean is one
    rounding of an exact half-sum (u |mean|), the difference one more (u |x - mean|), the variance two squares of that
    difference, a rounded sum and a rounded factor (5 u, so 2.5 u under the root), the quotient one rounding:
    (u |mean| + u |x - mean|) / den + 3.5 u |x_norm|, and one u on each term for the second order."""
    c = D.bn_case(N, C, S)
    r = D.run_bn(c, N, C, S, 1, 1)
    x = c["x"].astype(np.float64)
    mean = x.mean((0, 2))
    var = ((x - mean[None, :, None]) ** 2).sum((0, 2)) / (N * S - 1)
    assert np.abs(r["mean"] - mean).max() <= 2e-7 * np.abs(x).max()
    assert np.abs(r["var"] - var).max() <= 4e-7 * var.max()
    den = (np.sqrt(var) + 1e-6)[None, :, None]
    xn = (x - mean[None, :, None]) / den
    if N * S > 2:
        assert np.abs(r["x_norm"] - xn).max() <= 2e-6 * np.abs(xn).max()
    else:
        u = 2.0 ** -24
        assert np.all(np.abs(r["x_norm"] - xn) <= 2 * u * (np.abs(mean)[None, :, None] + np.abs(x - mean[None, :, None])) / den + 4.5 * u * np.abs(xn))
    assert np.allclose(r["rolling_mean"], .9 * c["rolling_mean"] + .1 * mean, rtol=0, atol=1e-6)
    lin = D.run_bn(c, N, C, S, 0, 0)
    assert np.array_equal(lin["out"], c["x"] + c["biases"][None, :, None]) and np.array_equal(lin["delta"], c["delta"])
    assert np.allclose(lin["bias_updates"], c["bias_updates"] + c["delta"].astype(np.float64).sum((0, 2)), rtol=0, atol=1e-5)


@pytest.mark.parametrize("bn, leaky", [(1, 1), (1, 0)])
@pytest.mark.parametrize("N, C, S", D.BN_SHAPES)
def test_host_batch_norm_backward_against_float64(N, C, S, bn, leaky):
    """The backward twin alone against Darknet's own formulas in float64 (F64Net.backward's: the leaky gradient keyed
    on the output, mean_delta, variance_delta, normalize_delta, with .00001 and the N * S divisor): not autograd, since
    Darknet's backward is not the derivative of its forward.  Both sides read the SAME float32 out, x, x_norm, mean
    and variance (the twin's forward), so the only difference is the backward's own rounding.

    The bound, from the operations, with u = 2^-24 and g the gradient (1, or .1f which is within u / 4 of .1).  The
    sums are float64 over float32 values and rounded once; a product of two float32 values is exact in float64.
      d1 = fl(delta g): 2 u (the rounding, the constant).          d2 = fl(d1 scale): 3 u.      xm = fl(x - mean): u.
      v = fl(var + .00001f): 2 u (the rounding, the constant), so 1 / sqrt(v) carries u and 1 / (v sqrt v) 3 u.
      bias_updates  = fl(b0 + fl(sum d1)): 2 u + u + u = 4 u on |b0| + sum|delta g|.
      scale_updates = fl(s0 + fl(sum d1 x_norm)): 4 u on |s0| + sum|delta g x_norm|.
      mean delta     md = fl(fl(sum d2) / -sqrt(v)): 3 u + u + u + u = 6 u on sum|delta g scale| / sqrt(v);
      variance delta vd = fl(fl(sum d2 xm) * -.5 / (v sqrt v)): (3 + 1) u + u + 3 u + u = 9 u on
                     sum|delta g scale (x - mean)| * .5 / (v sqrt v).
      delta = fl(a + b + c), a = d2 / (sqrt(var) + .00001f): 3 u + u (the constant) + u (the last rounding) = 5 u |a|;
              b = vd 2 xm / count: vd's own error E_vd, u of xm, u of the last rounding: (E_vd + 2 u |vd|) 2 |x - mean| / count;
              c = fl(md / count): E_md, u of the division, u of the last rounding: (E_md + 2 u |md|) / count.
    Every bound gets one more u on its magnitude for the second-order terms and the float64 sums (count 2^-53)."""
    u = 2.0 ** -24
    c = D.bn_case(N, C, S)
    r = D.run_bn(c, N, C, S, bn, leaky)
    f = lambda a: np.asarray(a, np.float64)
    col = lambda a: f(a)[None, :, None]
    cnt = N * S
    g = np.where(f(r["out"]) > 0, 1.0, .1) if leaky else np.ones((N, C, S))
    x, mean, var, scale = f(c["x"]), col(r["mean"]), col(r["var"]), col(c["scales"])
    d = f(c["delta"]) * g
    ad = np.abs(d)
    sums = lambda a: a.sum((0, 2), keepdims=True)
    exact = f(c["bias_updates"]) + sums(d)[0, :, 0]
    assert np.all(np.abs(r["bias_updates"] - exact) <= 5 * u * (np.abs(f(c["bias_updates"])) + sums(ad)[0, :, 0]))
    exact = f(c["scale_updates"]) + sums(d * f(r["x_norm"]))[0, :, 0]
    assert np.all(np.abs(r["scale_updates"] - exact) <= 5 * u * (np.abs(f(c["scale_updates"])) + sums(ad * np.abs(f(r["x_norm"])))[0, :, 0]))
    d, ad = d * scale, ad * np.abs(scale)
    xm = x - mean
    md = sums(d) * (-1. / np.sqrt(var + 1e-5))
    vd = sums(d * xm) * -.5 * (var + 1e-5) ** -1.5
    e_md = 7 * u * sums(ad) / np.sqrt(var + 1e-5)
    e_vd = 10 * u * sums(ad * np.abs(xm)) * .5 * (var + 1e-5) ** -1.5
    assert np.all(np.abs(col(r["stat"][0]) - md) <= e_md) and np.all(np.abs(col(r["stat"][1]) - vd) <= e_vd)
    a, b, cc = d / (np.sqrt(var) + 1e-5), vd * 2. * xm / cnt, md / cnt
    exact = a + b + cc
    bound = (5 * u * np.abs(a) + (e_vd + 2 * u * np.abs(vd)) * 2 * np.abs(xm) / cnt + (e_md + 2 * u * np.abs(md)) / cnt +
             u * (np.abs(a) + np.abs(b) + np.abs(cc)))
    worst = float((np.abs(r["delta"] - exact) / bound).max())
    print("bn backward %s leaky %d: worst |delta - exact| / bound %.3f" % ((N, C, S), leaky, worst))
    assert worst <= 1.0


def test_batch_of_one_value_is_an_argument_error():
    c = D.bn_case(1, 4, 1)
    with pytest.raises(_lib.BetaposeHipError, match="batch \\* spatial"):
        D.run_bn(c, 1, 4, 1, 1, 1)


def test_the_library_still_exports_what_the_header_declares():
    import helpers
    assert {"bp_train_conv", "bp_train_conv_host", "bp_train_bn_forward", "bp_train_bn_backward", "bp_train_update",
            "bp_train_update_host"} <= helpers.header_names() == set(_lib.PROTOTYPES)
