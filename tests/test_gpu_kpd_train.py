"""The key-point detector's training kernels on the device (csrc/kpd_train.hip, and the GEMM core at the stem's and the
Linears' shapes) against their host twins bit for bit -- outputs pre-filled with NaN, every call twice and once on a
second stream -- whole iterations against the reference's bars of tests/golden/kpd_train.npz, one full-size iteration
against a torch mirror in float64, and train_kpd.py end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kpd_train_common as K

pytestmark = pytest.mark.gpu
ROOT = K.ROOT


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream()


def three_runs(run, want, dev, side):
    for k in range(3):
        got = run(dev, side if k == 2 else None)
        for name, v in want.items():
            assert np.array_equal(K.bits(got[name]), K.bits(v)), (name, k)


@pytest.mark.parametrize("bn, relu", [(1, 0), (1, 1), (0, 1)], ids=["bn", "bn_relu", "bias_relu"])
@pytest.mark.parametrize("N, C, S", K.BN_SHAPES)
def test_batch_norm_equals_the_host_twin(N, C, S, bn, relu, dev, side):
    c = K.bn_case(N, C, S)
    three_runs(lambda d, s: K.run_bn(c, N, C, S, bn, relu, 1, d, s), K.run_bn(c, N, C, S, bn, relu), dev, side)


def test_batch_norm_with_running_statistics_equals_the_host_twin(dev, side):
    c = K.bn_case(3, 4, 12)
    three_runs(lambda d, s: K.run_bn(c, 3, 4, 12, 1, 1, 0, d, s), K.run_bn(c, 3, 4, 12, 1, 1, 0), dev, side)


def test_one_value_per_channel_is_an_argument_error_on_the_device(dev):
    from betapose_amd import _lib
    with pytest.raises(_lib.BetaposeHipError, match="more than one value per channel"):
        K.run_bn(K.bn_case(1, 4, 1), 1, 4, 1, 1, 1, 1, dev)


@pytest.mark.parametrize("gate", [0, 1], ids=["plain", "se"])
@pytest.mark.parametrize("N, C, S", K.BN_SHAPES)
def test_block_tail_equals_the_host_twin(N, C, S, gate, dev, side):
    c = K.tail_case(N, C, S)
    three_runs(lambda d, s: K.run_tail(c, N, C, S, gate, d, s), K.run_tail(c, N, C, S, gate), dev, side)


@pytest.mark.parametrize("S", K.POOL_S)
def test_se_pool_equals_the_host_twin(S, dev, side):
    rng = np.random.default_rng(S)
    y, dpool, dy0 = rng.standard_normal((5, S)).astype(np.float32), rng.standard_normal(5).astype(np.float32), rng.standard_normal((5, S)).astype(np.float32)
    three_runs(lambda d, s: K.run_pool(y, dpool, dy0, d, s), K.run_pool(y, dpool, dy0), dev, side)


def test_sigmoid_equals_the_host_twin(dev, side):
    x = np.concatenate([np.array([0, 30, -30, 700, -700], np.float32), np.random.default_rng(0).standard_normal(300).astype(np.float32) * 4])
    g = np.random.default_rng(1).standard_normal(x.size).astype(np.float32)
    want = K.run_sigmoid(x, g)
    assert want["s"][0] == 0.5 and want["s"][3] == 1 and want["s"][4] == 0
    three_runs(lambda d, s: K.run_sigmoid(x, g, d, s), want, dev, side)


@pytest.mark.parametrize("kind", ["random", "constant", "negative"])
@pytest.mark.parametrize("P, H, W", K.MAXPOOL_SHAPES)
def test_max_pool_equals_the_host_twin(P, H, W, kind, dev, side):
    rng = np.random.default_rng([P, H, W])
    x = {"random": rng.standard_normal((P, H, W)), "constant": np.full((P, H, W), 2.0), "negative": -1 - rng.uniform(0, 1, (P, H, W))}[kind].astype(np.float32)
    dout = rng.standard_normal((P, (H - 1) // 2 + 1, (W - 1) // 2 + 1)).astype(np.float32)
    want = K.run_maxpool(x, dout)
    if kind == "negative":
        assert (want["out"] < 0).all()          # the padding is -inf, not 0
    if kind == "constant":                      # ties pick the first index: the window's first tap inside the map
        oy, ox = np.mgrid[0:want["arg"].shape[1], 0:want["arg"].shape[2]]
        assert np.array_equal(want["arg"][0], np.maximum(2 * oy - 1, 0) * W + np.maximum(2 * ox - 1, 0))
        assert np.isclose(want["dx"].sum(), dout.sum(), atol=1e-4)
    three_runs(lambda d, s: K.run_maxpool(x, dout, d, s), want, dev, side)


@pytest.mark.parametrize("shape", K.CONV7_SHAPES + K.LINEAR_SHAPES, ids=[s[0] for s in K.CONV7_SHAPES + K.LINEAR_SHAPES])
def test_stem_and_linear_gemms_equal_the_host_twin(shape, dev, side):
    c = K.conv_case(shape)
    three_runs(lambda d, s: K.run_conv(c, shape, d, s), K.run_conv(c, shape), dev, side)


@pytest.mark.parametrize("h", K.RMSPROP_SETTINGS, ids=["plain", "momentum_decay", "decay", "momentum"])
def test_rmsprop_equals_the_host_twin(h, dev, side):
    rows = K.rmsprop_case()
    want = K.run_rmsprop(rows, h)
    assert all(np.isfinite(r["p"]).all() for r in want)
    for k in range(3):
        got = K.run_rmsprop(rows, h, dev, side if k == 2 else None)
        for a, b in zip(got, want):
            K.same_bits(a, b)
    if h["momentum"] == 0:
        assert all(np.array_equal(b["b"], r["b"]) for b, r in zip(want, rows))      # the buffer is left alone


@pytest.mark.parametrize("it", range(3))
@pytest.mark.parametrize("setting", [0, 1], ids=["defaults", "momentum_decay"])
def test_teacher_forced_iteration_equals_the_host_twin_and_meets_the_reference_bars(setting, it, dev):
    qh = K.teacher_forced(K.make_net(setting), setting, it)
    qg = K.teacher_forced(K.make_net(setting, dev), setting, it)
    K.same_bits(qg, qh)
    K.check_teacher_forced(qg, setting, it)


def test_validation_batch_equals_the_host_twin_and_meets_the_reference_bars(dev):
    rh, rg = K.validate(K.make_net(0)), K.validate(K.make_net(0, dev))
    assert rh[:2] == rg[:2] and np.array_equal(K.bits(rh[2]), K.bits(rg[2]))
    K.check_validate(rg)


def test_free_run_equals_the_host_twin_and_halves_the_loss(dev):
    host, gpu = K.make_net(0), K.make_net(0, dev)
    rh, rg = K.free_run(host), K.free_run(gpu)
    assert rh == rg and rg[-1][0] < 0.5 * rg[0][0], (rh, rg)
    K.same_bits({k: v.numpy() for k, v in gpu.state_dict().items()}, {k: v.numpy() for k, v in host.state_dict().items()})
    K.same_bits(gpu.optimizer_state(), host.optimizer_state())


def test_train_step_does_a_single_read_back(dev, monkeypatch):
    """no tensor but the stacked loss and accuracy leaves the device during train_step"""
    import torch
    net = K.make_net(0, dev)
    K.load(net, 0, 0)
    inps, labels, mask = (torch.from_numpy(a).to(dev) for a in K.batch(0))
    net.train_step(inps, labels, mask)         # allocates
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), real(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("item() read a tensor back"))
    monkeypatch.setattr(torch.Tensor, "tolist", (lambda real_tolist: lambda self: (pytest.fail("tolist() on a device tensor")
                                                                                    if self.is_cuda else real_tolist(self)))(torch.Tensor.tolist))
    monkeypatch.setattr(torch.Tensor, "numpy", (lambda real_numpy: lambda self, *a, **k: (pytest.fail("numpy() on a device tensor")
                                                                                          if self.is_cuda else real_numpy(self, *a, **k)))(torch.Tensor.numpy))
    loss, acc = net.train_step(inps, labels, mask)
    monkeypatch.undo()
    assert reads == [(2,)] and np.isfinite(loss) and 0 <= acc <= 1


def test_full_size_iteration_against_the_torch_mirror_in_float64(dev):
    """One iteration of the default net at batch 1, 320 x 256, on the device: the output and every gradient against the
    torch mirror in float64 on the device; the bar of each is 4 x the error of the mirror's own float32 autograd against
    that float64 run (at least 2^-23), measured here from torch.  Worst distance / bar seen on an MI355X: DESIGN.md 3.14."""
    import torch
    from betapose_amd.kpd_train import TrainableFastPose
    net = TrainableFastPose(device=dev, seed=3)
    rng = np.random.default_rng(7)
    inps = torch.from_numpy(rng.standard_normal((1, 3, 320, 256)).astype(np.float32)).to(dev)
    gout = torch.from_numpy(rng.standard_normal((1, 50, 80, 64)).astype(np.float32) * np.float32(1e-3)).to(dev)
    out = net.forward(inps, train=True).clone()
    net.zero_grad()
    net.backward(gout)

    def mirror(dtype):
        P = {k: v.to(dtype).requires_grad_(k in net.G) for k, v in net.P.items()}
        o = K.mirror_forward(P, inps.to(dtype), net.stages, True)
        o.backward(gout.to(dtype))
        return o.detach(), {k: P[k].grad for k in net.G}

    o64, g64 = mirror(torch.float64)
    o32, g32 = mirror(torch.float32)

    def dist(a, ref):
        return float((a.to(torch.float64) - ref).abs().max() / ref.abs().max().clamp_min(1e-300))

    worst = [("output", dist(out, o64) / max(4 * dist(o32, o64), K.FLOOR))]
    for k in net.G:
        worst.append((k, dist(net.G[k], g64[k]) / max(4 * dist(g32[k], g64[k]), K.FLOOR)))
    worst.sort(key=lambda t: -t[1])
    print("worst distance / bar:", worst[:5])
    assert worst[0][1] <= 1, worst[:5]


def test_train_kpd_writes_a_model_the_inference_net_loads(tmp_path):
    """train_kpd.py on a synthetic three-frame annotation, six epochs, so epoch 5 validates and saves; InferenNet_fast
    then loads model_5.pkl in a fresh child process"""
    from PIL import Image
    rng = np.random.default_rng(0)
    img = tmp_path / "img"
    img.mkdir()
    names = []
    for i in range(3):
        names.append("%04d.png" % i)
        Image.fromarray(rng.integers(0, 256, (96, 128, 3)).astype(np.uint8)).save(str(img / names[-1]))
    part = rng.uniform(30, 80, (3, 50, 2))
    bnd = np.array([[[20, 15, 100, 90]]] * 3, np.float64)
    L = max(len(n) for n in names)
    np.savez(str(tmp_path / "annot.npz"), bndbox=bnd, part=part, imgname=np.array([[ord(ch) for ch in n.ljust(L)] for n in names], np.int64))
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = tmp_path / "exp" / "try"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_kpd.py"), "--annot_train", str(tmp_path / "annot.npz"), "--annot_eval",
                        str(tmp_path / "annot.npz"), "--img_folder", str(img), "--out_dir", str(tmp_path / "exp"), "--expID", "try",
                        "--nEpochs", "6", "--trainBatch", "3",
                        "--validBatch", "3", "--seed", "1", "--device", "cuda:0"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Train-5 epoch | loss:" in r.stdout and "Valid-5 epoch | loss:" in r.stdout and "epoch is the best!" in r.stdout
    assert (out / "model_5.pkl").exists() and (out / "optimizer_5.npz").exists()
    import shutil
    shutil.copy(str(out / "model_5.pkl"), str(out / "seq1_model.pkl"))
    code = ("import sys, torch\nfrom betapose_amd.kpd import InferenNet_fast\nm = InferenNet_fast(5, 1, None, model_dir=sys.argv[1]).cuda().eval()\n"
            "y = m(torch.zeros(1, 3, 320, 256, device='cuda:0'))\nassert tuple(y.shape) == (1, 50, 80, 64) and bool(torch.isfinite(y).all())\nprint('loaded')\n")
    r = subprocess.run([sys.executable, "-c", code, str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "loaded" in r.stdout, r.stdout + r.stderr
