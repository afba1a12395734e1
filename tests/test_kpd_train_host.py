"""The key-point detector's training iteration on the host twins (no GPU): the recorded iterations of
tests/golden/kpd_train.npz teacher-forced against the reference's bars, each host kernel against float64, the RMSprop twin
against torch.optim.RMSprop live, the state dict and its file, the argument errors and the C ABI.

Tolerances of the per-kernel checks, for inputs of order 1: a float32 result carries its own rounding (2^-24 relative)
and that of the stored float32 mean and invstd (2^-24 relative each, entering every element), and a batch-norm gradient
is a difference of three terms of the size of the largest, so a result is held to 2^-20 of the largest reference value
(16 float32 roundings); the statistics themselves, float64 sums rounded once, to 2^-22."""
import os

import numpy as np
import pytest

import kpd_train_common as K
from betapose_amd import _lib

TOL, TOL_STAT = 2.0 ** -20, 2.0 ** -22


def close(ours, ref, tol=TOL):
    ref = np.asarray(ref, np.float64)
    d = float(np.abs(np.asarray(ours, np.float64) - ref).max())
    assert d <= tol * max(float(np.abs(ref).max()), 1e-30), (d, float(np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------ the recorded iterations
@pytest.mark.parametrize("it", range(3))
@pytest.mark.parametrize("setting", [0, 1], ids=["defaults", "momentum_decay"])
def test_teacher_forced_iteration_meets_the_reference_bars(setting, it):
    K.check_teacher_forced(K.teacher_forced(K.make_net(setting), setting, it), setting, it)


def test_validation_batch_meets_the_reference_bars():
    K.check_validate(K.validate(K.make_net(0)))


def test_free_run_halves_the_loss():
    """20 iterations over the recorded batches: the loss ends below half its first value (free-running parameters are not
    compared with the reference: RMSprop's first steps are sign-like)"""
    run = K.free_run(K.make_net(0))
    assert all(np.isfinite(l) for l, _ in run) and run[-1][0] < 0.5 * run[0][0], run


def test_train_step_is_the_pieces_in_the_reference_order():
    """train_step = forward, loss, zero_grad, backward, step: the same bits as the pieces called one by one"""
    a, b = K.make_net(1), K.make_net(1)
    K.load(a, 1, 0), K.load(b, 1, 0)
    inps, labels, mask = K.batch(0)
    la = a.train_step(inps, labels, mask)
    b.G["conv_out.bias"][...] = 3          # a stale gradient: zero_grad must clear it
    out = b.forward(inps, train=True)
    loss, acc, grad = b._loss(out, labels, mask, True)
    b.zero_grad()
    b.backward(grad)
    b.update()
    assert la == (loss, acc)
    K.same_bits({k: v.numpy() for k, v in a.state_dict().items()}, {k: v.numpy() for k, v in b.state_dict().items()})
    K.same_bits(a.optimizer_state(), b.optimizer_state())


# ------------------------------------------------------------------------------------------------ kernels against float64
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N, C, S", K.BN_SHAPES)
def test_host_batch_norm_against_torch_float64(N, C, S, relu):
    import torch
    c = K.bn_case(N, C, S)
    r = K.run_bn(c, N, C, S, 1, relu)
    t = {k: torch.from_numpy(v.astype(np.float64)) for k, v in c.items()}
    x, w, b = t["x"].requires_grad_(), t["w"].requires_grad_(), t["b"].requires_grad_()
    rm, rv = t["rm"].clone(), t["rv"].clone()
    y = torch.nn.functional.batch_norm(x, rm, rv, w, b, training=True, momentum=0.1, eps=1e-5)
    y = torch.relu(y) if relu else y
    y.backward(t["dy"])
    xd = c["x"].astype(np.float64)
    mean, var = xd.mean((0, 2)), xd.var((0, 2))
    close(r["mean"], mean, TOL_STAT), close(r["invstd"], 1 / np.sqrt(var + 1e-5), TOL_STAT)
    close(r["rm"], rm.numpy(), TOL_STAT), close(r["rv"], rv.numpy(), TOL_STAT)
    close(r["out"], y.detach().numpy())
    # the gradient's three terms, each of which carries its own roundings whatever is left of their difference
    inv = 1 / np.sqrt(var + 1e-5)
    xh = (xd - mean[None, :, None]) * inv[None, :, None]
    m = c["dy"].astype(np.float64) * ((y.detach().numpy() > 0) if relu else 1)
    terms = (np.abs(m) + np.abs(m.mean((0, 2)))[None, :, None] + np.abs(xh) * np.abs((m * xh).mean((0, 2)))[None, :, None]) \
        * (inv * np.abs(c["w"]))[None, :, None]
    assert np.abs(r["d"] - x.grad.numpy()).max() <= TOL * terms.max()
    close(r["gw"] - np.float32(0.25), w.grad.numpy()), close(r["gb"] + np.float32(0.5), b.grad.numpy())


def test_host_running_statistics_normalise_in_evaluation_and_bias_only_form():
    N, C, S = 3, 4, 10
    c = K.bn_case(N, C, S)
    r = K.run_bn(c, N, C, S, 1, 1, train=0)
    x = c["x"].astype(np.float64)
    y = (x - c["rm"][None, :, None]) / np.sqrt(c["rv"].astype(np.float64) + 1e-5)[None, :, None] * c["w"][None, :, None] + c["b"][None, :, None]
    close(r["out"], np.maximum(y, 0))
    assert np.array_equal(r["rm"], c["rm"]) and np.array_equal(r["rv"], c["rv"])
    for relu in (0, 1):
        lin = K.run_bn(c, N, C, S, 0, relu)
        y = c["x"] + c["b"][None, :, None]
        assert np.array_equal(lin["out"], np.maximum(y, 0) if relu else y)
        d = c["dy"] * (y > 0) if relu else c["dy"]
        assert np.array_equal(lin["d"], d.astype(np.float32))
        close(lin["gb"] + np.float32(0.5), d.astype(np.float64).sum((0, 2)))


def test_one_value_per_channel_is_an_argument_error():
    with pytest.raises(_lib.BetaposeHipError, match="more than one value per channel"):
        K.run_bn(K.bn_case(1, 4, 1), 1, 4, 1, 1, 1)


@pytest.mark.parametrize("gate", [0, 1], ids=["plain", "se"])
@pytest.mark.parametrize("N, C, S", [(2, 3, 1), (3, 5, 7), (2, 3, 132)])
def test_host_block_tail_against_float64(N, C, S, gate):
    c = K.tail_case(N, C, S)
    r = K.run_tail(c, N, C, S, gate)
    y, res, dout = (c[k].astype(np.float64) for k in ("y", "res", "dout"))
    s = c["s"].astype(np.float64)[:, :, None] if gate else 1.0
    out = np.maximum(y * s + res, 0)
    m = dout * (out > 0)
    close(r["out"], out), close(r["dres"], c["dres"] + m), close(r["dy"], m * s)
    if gate:
        close(r["ds"], (m * y).sum(2))


@pytest.mark.parametrize("S", K.POOL_S)
def test_host_se_pool_against_float64(S):
    rng = np.random.default_rng(S)
    y, dpool, dy0 = rng.standard_normal((3, S)).astype(np.float32), rng.standard_normal(3).astype(np.float32), rng.standard_normal((3, S)).astype(np.float32)
    r = K.run_pool(y, dpool, dy0)
    close(r["pool"], y.astype(np.float64).mean(1), TOL_STAT)
    close(r["dy"], dy0 + dpool.astype(np.float64)[:, None] / S, TOL_STAT)


def test_host_sigmoid_at_zero_and_in_the_tails():
    x = np.array([0, 30, -30, 700, -700, 1.5, -0.25], np.float32)
    g = np.linspace(-1, 1, len(x)).astype(np.float32)
    r = K.run_sigmoid(x, g)
    ref = 1 / (1 + np.exp(-x.astype(np.float64)))
    assert r["s"][0] == 0.5 and r["s"][1] == 1 and r["s"][3] == 1 and r["s"][4] == 0 and 0 < r["s"][2] < 1e-12
    close(r["s"], ref, TOL_STAT)
    assert np.abs(r["g"] - g * (1 - ref) * ref).max() <= TOL_STAT


@pytest.mark.parametrize("P, H, W", K.MAXPOOL_SHAPES)
def test_host_max_pool_against_torch(P, H, W):
    import torch
    rng = np.random.default_rng([P, H, W])
    x = rng.permutation(P * H * W).reshape(P, H, W).astype(np.float32) - np.float32(P * H * W)      # distinct, all negative
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dout = rng.standard_normal((P, OH, OW)).astype(np.float32)
    r = K.run_maxpool(x, dout)
    t = torch.from_numpy(x.astype(np.float64))[None].requires_grad_()
    y, idx = torch.nn.functional.max_pool2d(t, 3, 2, 1, return_indices=True)
    y.backward(torch.from_numpy(dout.astype(np.float64))[None])
    assert np.array_equal(r["out"], y[0].detach().numpy().astype(np.float32))      # all negative: a zero padding would win
    assert np.array_equal(r["arg"], idx[0].numpy())
    close(r["dx"], t.grad[0].numpy(), TOL_STAT)


def test_host_max_pool_ties_pick_the_first_index():
    x = np.full((1, 5, 5), 2.0, np.float32)
    dout = np.arange(1, 10, dtype=np.float32).reshape(1, 3, 3)
    r = K.run_maxpool(x, dout)
    first = np.array([[0, 1, 3], [5, 6, 8], [15, 16, 18]])      # the window's top-left tap inside the map
    assert np.array_equal(r["arg"][0], first)
    want = np.zeros(25, np.float32)
    want[first.reshape(-1)] = dout.reshape(-1)
    assert np.array_equal(r["dx"].reshape(-1), want)


@pytest.mark.parametrize("shape", K.CONV7_SHAPES + K.LINEAR_SHAPES, ids=[s[0] for s in K.CONV7_SHAPES + K.LINEAR_SHAPES])
def test_host_convolution_chain_against_float64(shape):
    """the 7 x 7 / 2 stem and the Linear as a 1 x 1 map in their three roles.  The longest chain has 147 (forward), 60
    (filter gradient) or 245 (input gradient) products of order-1 values: a float32 fmaf chain of n terms is held to
    n * 2^-24 of the sum of the products' magnitudes."""
    import torch
    _, N, C, H, W, Kc, size, stride = shape
    c = K.conv_case(shape)
    r = K.run_conv(c, shape)
    x, w = torch.from_numpy(c["x"].astype(np.float64)).requires_grad_(), torch.from_numpy(c["w"].astype(np.float64)).requires_grad_()
    y = torch.nn.functional.conv2d(x, w, stride=stride, padding=size // 2)
    y.backward(torch.from_numpy(c["dy"].astype(np.float64)))
    a = torch.nn.functional.conv2d(x.detach().abs(), w.detach().abs(), stride=stride, padding=size // 2)
    a.requires_grad_(False)
    xa, wa = x.detach().abs().requires_grad_(), w.detach().abs().requires_grad_()
    torch.nn.functional.conv2d(xa, wa, stride=stride, padding=size // 2).backward(torch.from_numpy(np.abs(c["dy"]).astype(np.float64)))
    n = 256 * 2.0 ** -24
    assert (np.abs(r["y"] - y.detach().numpy()) <= n * a.numpy() + 1e-30).all()
    assert (np.abs(r["dw"] - c["dw0"] - w.grad.numpy()) <= n * (wa.grad.numpy() + np.abs(c["dw0"])) + 1e-30).all()
    assert (np.abs(r["dx"] - c["dx0"] - x.grad.numpy()) <= n * (xa.grad.numpy() + np.abs(c["dx0"])) + 1e-30).all()


def test_the_older_entry_point_still_refuses_size_seven():
    c = K.conv_case(K.CONV7_SHAPES[0])
    with pytest.raises(_lib.BetaposeHipError, match="size must be 1 or 3"):
        _lib.check(_lib.lib().bp_train_conv_host(0, _lib.ptr(c["x"]), _lib.ptr(c["w"]), _lib.ptr(np.zeros_like(c["dy"])), 2, 3, 9, 11, 5, 7, 2, None))
    assert _lib.lib().bp_train_conv_scratch(2, 3, 9, 11, 5, 7, 2) == 0 < _lib.lib().bp_kpd_train_conv_scratch(2, 3, 9, 11, 5, 7, 2)


def update_bars():
    """the fixture's bars of the update, one per kind: 4 x the worst ref_err of the recorded parameters (p), of square_avg
    (v) and of the momentum buffers (b), each for its own kind only"""
    g, m = K.golden(), K.meta()
    pk = set(m["param_keys"])
    worst = dict(p=0.0, v=0.0, b=0.0)
    for k, v in g.items():
        if k.startswith("err.s") and k.endswith(".V"):
            worst["v"] = max(worst["v"], float(np.max(v)))
        elif k.startswith("err.s") and k.endswith(".B"):
            worst["b"] = max(worst["b"], float(np.max(v)))
        elif k.startswith("err.s") and k.endswith(".P"):
            worst["p"] = max(worst["p"], max(float(e) for key, e in zip(m["keys"], v) if key in pk))
    return {k: max(4 * v, K.FLOOR) for k, v in worst.items()}


@pytest.mark.parametrize("h", K.RMSPROP_SETTINGS, ids=["plain", "momentum_decay", "decay", "momentum"])
def test_host_rmsprop_against_torch_live(h):
    """two consecutive steps of the twin against torch.optim.RMSprop on the same float32 tensors"""
    import torch
    rows = K.rmsprop_case()
    params = [torch.nn.Parameter(torch.from_numpy(r["p"].copy())) for r in rows]
    opt = torch.optim.RMSprop(params, lr=h["lr"], alpha=h["alpha"], eps=h["eps"], weight_decay=h["wd"], momentum=h["momentum"])
    for p, r in zip(params, rows):      # start from a non-trivial optimiser state
        opt.state[p] = dict(step=torch.tensor(0.0), square_avg=torch.from_numpy(r["v"].copy()))
        if h["momentum"] > 0:
            opt.state[p]["momentum_buffer"] = torch.from_numpy(r["b"].copy())
    bar = update_bars()
    print(bar)
    for step in range(2):
        for p, r in zip(params, rows):
            p.grad = torch.from_numpy(r["g"].copy())
        opt.step()
        rows = K.run_rmsprop(rows, h)
        for p, r in zip(params, rows):
            assert np.isfinite(r["p"]).all()
            dp, dv = K.distance(r["p"], p.detach().numpy()), K.distance(r["v"], opt.state[p]["square_avg"].numpy())
            print(step, len(r["p"]), dp, dv)
            assert dp <= bar["p"] and dv <= bar["v"], (dp, dv, bar)
            if h["momentum"] > 0:
                db = K.distance(r["b"], opt.state[p]["momentum_buffer"].numpy())
                assert db <= bar["b"], (db, bar)


# ------------------------------------------------------------------------------------------------ state, files, errors
@pytest.fixture(scope="module")
def default_net():
    from betapose_amd.kpd_train import TrainableFastPose
    return TrainableFastPose()


def test_state_dict_has_the_reference_keys_shapes_and_dtypes(default_net):
    import json
    want = json.loads(bytes(K.golden()["full_state_dict"]).decode())
    sd = default_net.state_dict()
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == want
    tiny = K.make_net(0).state_dict()
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in tiny.items()] == K.meta()["state_dict"]


def test_saved_pkl_loads_as_the_inference_stream(default_net, tmp_path):
    import torch
    from betapose_amd import weights as W
    path = str(tmp_path / "model_5.pkl")
    sd = default_net.state_dict()
    torch.save(sd, path)
    back = W.load_kpd_pkl(path)
    assert list(back) == list(sd) and back["preact.bn1.num_batches_tracked"].dtype == np.int64
    stream = W.fastpose_stream_from_state_dict(back)
    assert stream.size == W.fastpose_stream_size() and stream.dtype == np.float32
    assert np.array_equal(stream[-50 * 128 * 9:], sd["conv_out.weight"].numpy().reshape(-1))


def test_initialisation_follows_torch_defaults():
    net = K.make_net(0, seed=5)
    w = net.P["preact.conv1.weight"]
    bound = 1 / np.sqrt(3 * 49)
    assert np.abs(w).max() <= bound and np.abs(w).max() > 0.8 * bound and abs(float(w.mean())) < 0.2 * bound
    assert np.array_equal(net.P["preact.bn1.weight"], np.ones(4, np.float32)) and np.array_equal(net.P["preact.bn1.running_var"], np.ones(4, np.float32))
    assert not np.any(net.P["preact.bn1.bias"]) and not np.any(net.P["preact.bn1.running_mean"])
    assert np.abs(net.P["conv_out.bias"]).max() <= 1 / 3.0
    other = K.make_net(0, seed=6)
    assert not np.array_equal(other.P["preact.conv1.weight"], w)


def test_adam_and_a_tail_that_does_not_divide_raise_errors_that_name_the_problem():
    from betapose_amd.kpd_train import TrainableFastPose
    with pytest.raises(ValueError, match="adam"):
        TrainableFastPose(2, ((2, 1, 1), (4, 1, 2)), 4, optMethod="adam")
    with pytest.raises(ValueError, match="multiple of 16"):
        TrainableFastPose(2, ((2, 1, 1), (2, 1, 2)), 4)


def test_the_library_exports_what_the_header_declares():
    import helpers
    names = {n for n in _lib.PROTOTYPES if n.startswith("bp_kpd_train_")}
    assert len(names) == 26 and names <= helpers.header_names() == set(_lib.PROTOTYPES)
    for n in names:
        assert hasattr(_lib.lib(), n), n


def test_the_fixture_stays_small():
    """The archive holds what the issue lists for two settings of three iterations (22 state-sized vectors of about 2 900
    float32 each, seven output maps of 2 048): about 80 000 incompressible float32 values, which no 200 KB archive holds.
    It is 334 915 bytes; the cap is the next multiple of 10 000, so anything added to it has to be argued for."""
    assert os.path.getsize(os.path.join(K.ROOT, "tests", "golden", "kpd_train.npz")) <= 340000
