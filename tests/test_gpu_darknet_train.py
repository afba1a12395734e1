"""The training iteration on the device (csrc/darknet_train.hip) against its host twins bit for bit -- uint32 views,
outputs pre-filled with a sentinel, every call twice and once on a second stream -- and whole steps against the
reference's bars of tests/golden/darknet_train.npz and, for the shipped topology, darknet_train_shipped.npz."""
import os
import subprocess
import sys

import numpy as np
import pytest

import darknet_train_common as D

pytestmark = pytest.mark.gpu
ROOT = D.ROOT


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream()


@pytest.mark.parametrize("role", [0, 1, 2], ids=["forward", "filter_grad", "input_grad"])
@pytest.mark.parametrize("shape", D.CONV_SHAPES, ids=[s[0] for s in D.CONV_SHAPES])
def test_gemm_role_equals_the_host_twin(shape, role, dev, side):
    """each role alone; the tensor the role writes is a view offset by one float; roles 1 and 2 add into non-zero values"""
    import torch
    x, w, dy, dx0, wu0 = D.conv_case(shape)
    hx, hw, hy = (dx0.copy() if role == 2 else x.copy()), (wu0.copy() if role == 1 else w.copy()), dy.copy()
    if role == 0:
        hy[...] = np.nan
    start = [hx.copy(), hw.copy(), hy.copy()]
    D.run_conv(role, shape, hx, hw, hy)
    want = (hy, hw, hx)[role]
    for run in range(3):
        t = []
        for i, a in enumerate(start):
            if i == (2, 1, 0)[role]:        # the written tensor: one float into a buffer with a sentinel on both sides
                buf = torch.full((a.size + 2,), -77.0, device=dev)
                buf[1:-1] = torch.from_numpy(a.reshape(-1)).to(dev)
                t.append((buf, buf[1:-1].view(a.shape)))
            else:
                t.append((None, torch.from_numpy(a).to(dev)))
        if run == 2:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                D.run_conv(role, shape, t[0][1], t[1][1], t[2][1], dev, side.cuda_stream)
            side.synchronize()
        else:
            D.run_conv(role, shape, t[0][1], t[1][1], t[2][1], dev)
        buf, out = t[(2, 1, 0)[role]]
        got = out.cpu().numpy()
        assert float(buf[0]) == -77.0 and float(buf[-1]) == -77.0, "a store outside the tensor"
        assert np.array_equal(_bits(got), _bits(want)), (shape[0], role, run, float(np.nanmax(np.abs(got - want))))
        for i in range(3):
            if i != (2, 1, 0)[role]:
                assert np.array_equal(_bits(t[i][1].cpu().numpy()), _bits(start[i]))


@pytest.mark.parametrize("role", [0, 1, 2], ids=["forward", "filter_grad", "input_grad"])
def test_gemm_role_on_subnormal_operands_equals_the_host_twin(role, dev):
    """c3_k18_3x3 with operands of about 2^-70: every product and partial sum is subnormal or zero.  The host twin's
    fmaf keeps subnormals; the fp32 matrix pipe has to as well for DESIGN.md 3.13's bit-for-bit claim to hold below
    2^-126.  It does on the MI355X: all three roles left the host twin's bits."""
    import torch
    shape, x, w, dy, dx0, wu0 = D.subnormal_conv_case()
    hx, hw, hy = (dx0.copy() if role == 2 else x.copy()), (wu0.copy() if role == 1 else w.copy()), dy.copy()
    if role == 0:
        hy[...] = np.nan
    t = [torch.from_numpy(a.copy()).to(dev) for a in (hx, hw, hy)]
    D.run_conv(role, shape, hx, hw, hy)
    want = (hy, hw, hx)[role]
    assert np.abs(want).max() < 2.0 ** -126 and np.count_nonzero(want) > want.size // 2, "the case is not subnormal"
    D.run_conv(role, shape, t[0], t[1], t[2], dev)
    got = t[(2, 1, 0)[role]].cpu().numpy()
    differ = _bits(got) != _bits(want)
    print("role %d: %d of %d elements differ, %d of them zero on the device, %d zero on the host"
          % (role, differ.sum(), differ.size, (got[differ] == 0).sum(), (want[differ] == 0).sum()))
    assert not differ.any()


@pytest.mark.parametrize("bn, leaky", [(1, 1), (0, 0), (0, 1)])
@pytest.mark.parametrize("N, C, S", D.BN_SHAPES)
def test_batch_norm_equals_the_host_twin(N, C, S, bn, leaky, dev, side):
    import torch
    c = D.bn_case(N, C, S)
    want = D.run_bn(c, N, C, S, bn, leaky)
    for run in range(3):
        if run == 2:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                got = D.run_bn(c, N, C, S, bn, leaky, dev, side.cuda_stream)
        else:
            got = D.run_bn(c, N, C, S, bn, leaky, dev)
        for k, v in want.items():
            assert np.array_equal(_bits(got[k]), _bits(v)), (k, run)


def test_batch_of_one_value_is_an_argument_error_on_the_device(dev):
    from betapose_amd import _lib
    with pytest.raises(_lib.BetaposeHipError, match="batch \\* spatial"):
        D.run_bn(D.bn_case(1, 4, 1), 1, 4, 1, 1, 1, dev)


def test_update_equals_the_host_twin_and_three_numpy_passes(dev, side):
    import torch
    from betapose_amd import _lib
    rows = D.update_case()
    a, dk, mom = np.float32(0.01) / np.float32(6), np.float32(-0.0005) * np.float32(6), np.float32(0.9)
    ref = D.update_reference(rows, a, dk, mom)
    chunk = int(_lib.lib().bp_train_update_chunk())
    blocks = sum((len(p) + chunk - 1) // chunk for p, _, _ in rows)
    for run in range(3):
        t = [(torch.from_numpy(p).to(dev), torch.from_numpy(u).to(dev), k) for p, u, k in rows]
        table = torch.tensor([(p.data_ptr(), u.data_ptr(), p.numel(), k) for p, u, k in t], dtype=torch.int64, device=dev)
        s = side if run == 2 else torch.cuda.current_stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _lib.check(_lib.lib().bp_train_update(table.data_ptr(), len(t), blocks, float(a), float(dk), float(mom), s.cuda_stream))
        s.synchronize()
        for (p, u, _), (rp, ru) in zip(t, ref):
            assert np.array_equal(_bits(p.cpu().numpy()), _bits(rp)) and np.array_equal(_bits(u.cpu().numpy()), _bits(ru))


@pytest.mark.parametrize("name", ["a0", "a1"])
def test_one_step_equals_the_host_twin_and_meets_the_reference_bars(name, dev):
    """group A on the device: every quantity equals the host twin's bit for bit and lies within the reference's bar"""
    qh, dh = D.group_a_step(D.make_net(name), name)
    qg, dg = D.group_a_step(D.make_net(name, dev), name)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(dh, dg))
    for q, v in qg.items():
        assert np.array_equal(_bits(v), _bits(qh[q])), q
        D.check(q, v)


def test_shipped_topology_step_equals_the_host_twin_and_meets_the_reference_bars(dev):
    """The step of test_darknet_train_host.py's shipped-topology test (cfg.yolov3_single_cfg_text(1) on 64 x 32, batch
    2, the reference's yolo deltas going in) on the device: every quantity and the heads' own deltas equal the host
    twin's bit for bit, and every quantity lies within the reference's bar of the float64 step.  Then a second call
    through train_step on the same batch, the deltas formed from the truth rows: the host twin's cost bit for bit."""
    import time
    qh, dh, mh, ih = D.shipped_host()
    net = D.shipped_net(dev)
    qg, dg, mg, ig = D.shipped_step(net)
    print("one step: host twin %.1f s, device (with its read-backs) %.1f s" % (ih["seconds"], ig["seconds"]))
    assert ig["rows"] == ih["rows"] == 222 and ig["blocks"] == ih["blocks"]
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(dh, dg))
    assert set(qg) == set(qh)
    for q, v in qg.items():
        assert np.array_equal(_bits(v), _bits(qh[q])), (q, float(np.abs(v - qh[q]).max()))
    assert all(np.array_equal(a, b) for a, b in zip(mh, mg) if a is not None)
    D.check_shipped(qg, "device")
    _, x, t = D.shipped_inputs()
    t0 = time.perf_counter()
    cost = np.float32(net.train_step(x, t))
    print("the second call: %.2f s on the device" % (time.perf_counter() - t0))
    assert _bits(cost) == _bits(D.shipped_host_second_cost()), (cost, D.shipped_host_second_cost())


def test_non_square_tiny_net_equals_the_host_twin(dev):
    """case a0's net on a 24 x 16 input (test_darknet_train_host.py holds the host twin to float64 there): one
    train_step on the device, every quantity and the heads' deltas bit for bit"""
    qh, dh = D.tiny_wide_step()
    qg, dg = D.tiny_wide_step(dev)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(dh, dg))
    assert set(qg) == set(qh) and len(qg) > 60
    for q, v in qg.items():
        assert np.array_equal(_bits(v), _bits(qh[q])), q


def test_subdivisions_equal_the_host_twin_and_meet_the_reference_bars(dev):
    """group B through train_step: every call's cost and state on the device equal the host twin's bit for bit, and lie
    within the reference's bars"""
    host, gpu = D.make_net("b"), D.make_net("b", dev)
    for k in range(D.meta()["cases"]["b"]["calls"]):
        inps, truth = D.case_batch("b", k)
        ch, cg = host.train_step(inps, truth), gpu.train_step(inps, truth)
        assert np.float32(ch) == np.float32(cg), (k, ch, cg)
        D.check("b.%d.cost" % k, np.float32(cg))
        sh, sg = host.state(), gpu.state()
        for q, v in sg.items():
            assert np.array_equal(_bits(v), _bits(sh[q])), (k, q, float(np.abs(v - sh[q]).max()))
            D.check("b.%d.post.%s" % (k, q), v)
        for lh, lg in zip(host.convs, gpu.convs):
            assert np.array_equal(_bits(lg["output"].cpu().numpy()), _bits(lh["output"]))


def test_train_step_reads_back_only_the_cost(dev, monkeypatch):
    """no tensor but the stacked costs leaves the device during train_step, and nothing is captured"""
    import torch
    net = D.make_net("a0", dev)
    inps, truth = D.case_batch("a0", 0)
    inps, truth = torch.from_numpy(inps).to(dev), torch.from_numpy(truth).to(dev)
    net.train_step(inps, truth)         # allocates
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), real(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("item() read a tensor back"))
    monkeypatch.setattr(torch.Tensor, "tolist", (lambda real_tolist: lambda self: (pytest.fail("tolist() on a device tensor")
                                                                                    if self.is_cuda else real_tolist(self)))(torch.Tensor.tolist))
    monkeypatch.setattr(torch.Tensor, "numpy", (lambda real_numpy: lambda self, *a, **k: (pytest.fail("numpy() on a device tensor")
                                                                                          if self.is_cuda else real_numpy(self, *a, **k)))(torch.Tensor.numpy))
    assert not torch.cuda.is_current_stream_capturing()
    cost = net.train_step(inps, truth)
    assert reads == [(len(net.heads),)] and np.isfinite(cost)


def test_train_detector_writes_weights_that_detector_map_reads(tmp_path):
    """train_detector.py --max_batches 3 on a dozen 64 x 64 frames, then detector_map.py on the file it wrote"""
    import yolo_train_common as Y
    lst = Y.write_folder(str(tmp_path / "data"), n=12, H=64, W=64)
    cfg = D.meta()["cases"]["a0"]["cfg"].replace("width=16\nheight=16", "width=64\nheight=64").replace("batch=3", "batch=4")
    (tmp_path / "net.cfg").write_text(cfg)
    (tmp_path / "obj.names").write_text("obj0\n")
    (tmp_path / "obj.data").write_text("classes = 1\ntrain = %s\nvalid = %s\nnames = %s\nbackup = %s\n"
                                       % (lst, lst, tmp_path / "obj.names", tmp_path / "backup"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_detector.py"), "--data", str(tmp_path / "obj.data"), "--cfg",
                        str(tmp_path / "net.cfg"), "--max_batches", "3", "--seed", "1", "--device", "cuda:0"], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if " avg loss, " in ln]
    assert len(lines) == 3 and lines[0].startswith(" 1: ") and lines[2].endswith("12 images"), r.stdout
    final = tmp_path / "backup" / "net_final.weights"
    assert final.exists() and (tmp_path / "backup" / "net_last.weights").exists() is False
    r = subprocess.run([sys.executable, os.path.join(ROOT, "detector_map.py"), "--data", str(tmp_path / "obj.data"), "--cfg",
                        str(tmp_path / "net.cfg"), "--weights", str(final)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "mean average precision (mAP)" in r.stdout, r.stdout + r.stderr
