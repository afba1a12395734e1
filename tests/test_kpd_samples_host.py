"""The host side of the KPD training samples (csrc/kpd_sample_host.cpp through the bp_*_host entry points,
betapose_amd/train_data.py, kpd_samples.py): the reference's own outputs from tests/golden/kpd_samples.npz (cropBox,
generateSampleBox whole, heatmapAccuracy, the float32 MSELoss), the rotation against F.grid_sample, the loss and its
gradient against torch, and the command-line tool.  No GPU.

Measured on the CPU when this file was written (each test prints its figure before it asserts):
  kpd_inputs vs cropBox / generateSampleBox   max |diff| 8.9e-8   (bar 1e-6)
  rotation vs grid_sample                     max |diff| 1.3e-6   (bar 2e-5)
  gradient vs torch autograd                  0 ulp of the largest gradient (bar 4)
  loss vs float64 MSELoss                     relative 2.5e-16 (bar 1e-12); vs the reference's float32 loss 2.9e-8 (bar 1e-5)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kpd_samples_common as kc
from betapose_amd import annotate as A, train_data as T

ROOT = kc.ROOT
EPS32 = float(np.finfo(np.float32).eps)


def ulps(a, b):
    """|a - b| in units of float32 spacing at b"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(b), np.float32(1e-30))).astype(np.float64)


def test_fixture_says_what_ran():
    g = kc.golden()
    meta = json.loads(str(g["meta"]))
    assert meta["conditions"]["exempt_cases"] == 0 and meta["conditions"]["corner_integer_margin_px"] == 1e-3
    assert any("generateSampleBox" in s for s in meta["reference_ran"]) and any("heatmapAccuracy" in s for s in meta["reference_ran"])
    assert any("SpecialCrop and Pad" in s for s in meta["restated"]) and meta["rotate"] == 0
    names = meta["sample_cases"]
    assert "eval" in names and "train flip" in names and "dpg patch" in names and "dpg normal" in names
    assert sum(n.startswith("dpg switch") for n in names) == 9
    assert g["s_inp"].shape == (len(names), 3, 20, 16) and g["s_out"].shape == (len(names), 7, 10, 8)
    for v in (g["s_ul0"], g["s_br0"], g["s_ul"], g["s_br"]):       # the generator's corner condition holds
        assert np.abs(v - np.rint(v)).min() > 1e-3
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kpd_samples.npz")) < 200 * 1024


@pytest.mark.parametrize("res", [(20, 16), (13, 10)])
def test_inputs_equal_cropbox(res):
    """Bar 1e-6 absolute: values are at most 0.6 in magnitude (one ulp 6e-8), and the two orders of at most seven
    rounded operations per pixel can differ by about 4.2e-7."""
    g = kc.golden()
    n = len(g["c_ul"])
    got = T.kpd_inputs(g["frames"], np.ones(n, np.int32), g["c_ul"], g["c_br"], None, None, res)
    want = g["c_inp_%dx%d" % res]
    assert got.shape == want.shape and got.dtype == np.float32
    worst = float(np.abs(got - want).max())
    print("kpd_inputs vs cropBox at %dx%d: max |diff| %.3g" % (res + (worst,)))
    assert worst <= 1e-6
    assert np.abs(want).max() > 0.3                                     # (not a comparison of zeros)


def _sample_inputs(g, i):
    train = bool(g["s_train"][i])
    gains = g["s_gains"][i:i + 1].astype(np.float32) if train else None
    blank = np.array([g["s_joint_num"][i] == 0], np.uint8)
    inp = T.kpd_inputs(g["frames"], g["s_frame"][i:i + 1].astype(np.int32), g["s_ul"][i:i + 1], g["s_br"][i:i + 1], gains, blank, (20, 16))
    flip = np.array([train and g["s_flip_draw"][i] < 0.5], np.uint8)
    return inp, flip


def test_inputs_equal_generatesamplebox():
    """The whole sample's ``inp``, evaluation and training mode, with and without addDPG; flipped where the reference
    flipped.  One sample has jointNum == 0 and is zero."""
    g = kc.golden()
    worst, flipped, blanks = 0.0, 0, 0
    for i in range(len(g["s_inp"])):
        inp, flip = _sample_inputs(g, i)
        inp = T.augment_maps(inp, flip, [0.0])
        worst = max(worst, float(np.abs(inp[0] - g["s_inp"][i]).max()))
        flipped += int(flip[0])
        if g["s_joint_num"][i] == 0:
            blanks += 1
            assert not inp.any() and not g["s_inp"][i].any()
    print("kpd_inputs vs generateSampleBox: max |diff| %.3g over %d samples (%d flipped, %d blank)" % (worst, len(g["s_inp"]), flipped, blanks))
    assert worst <= 1e-6 and flipped >= 2 and blanks == 1


def test_blank_and_gains_optional():
    g = kc.golden()
    ul, br = kc.window_cases(48, 64)
    idx = np.zeros(len(ul), np.int32)
    blank = np.zeros(len(ul), np.uint8)
    blank[1] = 1
    got = T.kpd_inputs(g["frames"], idx, ul, br, None, blank, (13, 10))
    assert not got[1].any() and got[0].any() and got[2].any()
    ones = T.kpd_inputs(g["frames"], idx, ul, br, np.ones((len(ul), 3), np.float32), blank, (13, 10))
    assert np.array_equal(got.view(np.uint32), ones.view(np.uint32))      # x * 1.0f == x: skipping the multiply changes no bit


def test_gain_clamp_exact():
    """Gains of exactly 0.7 and 1.3 over pixels of 0 and 255: a window of the input's own size makes the resize the
    identity (every weight is 0 or 1), so each output is one tap, bit for bit."""
    fr = kc.frames_of(48, 64)[:1]
    ul, br = np.array([[2.0, 4.0]] * 2, np.float32), np.array([[18.0, 24.0]] * 2, np.float32)
    gains = np.array([[0.7, 1.3, 0.7], [1.3, 0.7, 1.3]], np.float32)
    got = T.kpd_inputs(fr, [0, 0], ul, br, gains, None, (20, 16))
    px = fr[0, 4:24, 2:18].astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    mean = np.array(T.MEAN_RGB, np.float32)[:, None, None]
    assert px.min() == 0 and px.max() == 1
    for b in range(2):
        want = np.clip(px * gains[b][:, None, None], np.float32(0), np.float32(1)) - mean
        assert np.array_equal(got[b].view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert (got[1, 0] == np.float32(1) - np.float32(0.406)).any()         # 255 * 1.3 was clamped to 1


def test_flip_and_shuffle_equal_the_reference_bitwise():
    """Labels: kpd_targets (bit-equal to transformBox / drawGaussian) through augment_maps with the golden's flipRef
    pairs equal the reference's ``out``; a flip is the reversed array."""
    g = kc.golden()
    flipped = 0
    for i in range(len(g["s_out"])):
        lab, _, mask = A.kpd_targets(g["s_part"][i:i + 1, :7], g["s_ul"][i:i + 1], g["s_br"][i:i + 1], (20, 16), (10, 8), want_mask=True)
        flip = np.array([bool(g["s_train"][i]) and g["s_flip_draw"][i] < 0.5], np.uint8)
        got = T.augment_maps(lab, flip, [0.0], kc.FLIP_PAIRS)
        assert np.array_equal(got[0].view(np.uint32), g["s_out"][i].view(np.uint32)), i
        assert np.array_equal(mask[0], g["s_setMask"][i])
        flipped += int(flip[0]) * int(got.any())
    assert flipped >= 2
    x = np.random.default_rng(0).normal(size=(2, 7, 13, 10)).astype(np.float32)
    y = T.augment_maps(x, [1, 0], [0.0, 0.0], kc.FLIP_PAIRS)
    perm = [1, 0, 2, 6, 4, 5, 3]
    assert np.array_equal(y[0], x[0][perm][:, :, ::-1]) and np.array_equal(y[1], x[1])
    assert T.channel_table(7, kc.FLIP_PAIRS).tolist() == perm


def test_dpg_windows_and_joint_count():
    """The recorded draws through kpd_windows / dpg_windows / joint_count: windows within 1 float32 ulp of the
    reference's, jointNum equal."""
    g = kc.golden()
    n = len(g["s_ul"])
    ul0, br0 = A.kpd_windows(g["s_bndbox"], g["s_scale_rate"], (48, 64))
    assert ulps(ul0, g["s_ul0"]).max() <= 1 and ulps(br0, g["s_br0"]).max() <= 1
    dpg = np.flatnonzero(g["s_dpg"])
    assert len(dpg) >= 11
    draws = {"patch_scale": g["s_patch_scale"][dpg], "patch_pos": g["s_patch_pos"][dpg], "normal": g["s_normal"][dpg],
             "switch": g["s_switch"][dpg]}
    ul, br, jn = T.dpg_windows(None, g["s_ul0"][dpg], g["s_br0"][dpg], g["s_part"][dpg], (48, 64), True, draws, g["s_bndbox"][dpg])
    worst = max(ulps(ul, g["s_ul"][dpg]).max(), ulps(br, g["s_br"][dpg]).max())
    print("dpg_windows: worst corner %.2f ulp" % worst)
    assert worst <= 1
    assert np.array_equal(jn, g["s_joint_num"][dpg]) and (jn > 13).sum() >= 9
    rest = np.flatnonzero(~g["s_dpg"].astype(bool))
    assert np.array_equal(T.joint_count(g["s_part"][rest], g["s_ul"][rest], g["s_br"][rest]), g["s_joint_num"][rest])
    assert len(rest) + len(dpg) == n
    # every halving was reached: the windows differ from the un-halved ones in the coordinates the switch names
    assert len({round(float(s), 2) for s in g["s_switch"][dpg] if s > 0}) >= 9


@pytest.mark.parametrize("shape", [(2, 3, 20, 16), (1, 7, 13, 10)])
def test_rotation_equals_grid_sample(shape):
    """Bar 2e-5 absolute for maps of at most 32 px: grid_sample forms its coordinates in float32 through the [-1, 1]
    normalisation, a few ulp of 32 (about 4e-6) each, against a slope of at most 1.1 per pixel."""
    rng = np.random.default_rng(2)
    x = rng.uniform(-0.55, 0.55, shape).astype(np.float32)
    worst = 0.0
    for angle in kc.ANGLES:
        for flip in (0, 1):
            y = T.augment_maps(x, [flip] * shape[0], [angle] * shape[0], kc.FLIP_PAIRS if shape[1] == 7 else ())
            perm = T.channel_table(7, kc.FLIP_PAIRS) if shape[1] == 7 else None
            for b in range(shape[0]):
                worst = max(worst, float(np.abs(y[b] - kc.rotate_reference(x[b], flip, angle, perm)).max()))
    print("rotation vs grid_sample at %s: max |diff| %.3g" % (shape, worst))
    assert worst <= 2e-5


def test_rotation_identities():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(3, 3, 20, 16)).astype(np.float32)
    x[0, 0, 0, 0] = -0.0
    y = T.augment_maps(x, [1, 1, 0], [0.0, 0.0, 0.0])
    assert np.array_equal(y[:2].view(np.uint32), np.ascontiguousarray(x[:2, :, :, ::-1]).view(np.uint32))
    assert np.array_equal(y[2].view(np.uint32), x[2].view(np.uint32))
    # a constant map stays the constant: the four weights sum to 1 up to their own rounding -- four products of two
    # roundings each and three additions, so at most 11 half-ulps; 8 ulp is the bar
    for c in (0.0, 1.0, -0.4375):
        k = np.full((1, 2, 13, 10), c, np.float32)
        for angle in kc.ANGLES[1:]:
            r = T.augment_maps(k, [0], [angle])
            assert np.abs(r - np.float32(c)).max() <= 8 * EPS32 * abs(c)


def _loss_cases():
    g = kc.golden()
    return {"a": (g["a_a_out"], g["a_a_labels"], g["a_a_mask"]), "b": (g["a_b_out"], g["a_b_labels"], g["a_b_mask"]),
            "c": (g["a_c_out"], g["a_c_labels"], g["a_c_mask"])}


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_loss_equals_mse(case):
    """Against torch.nn.MSELoss evaluated in float64 (relative 1e-12) -- of the residual ``out * setMask - labels`` that
    the definition forms in float32, as the reference does: a float64 residual would differ from any float32 one by
    about 1e-8 relative, so it is the squares and their sum that are checked at 1e-12.  And against the reference's own
    float32 loss (relative 1e-5: a float32 sum of at most 10^4 terms can be off by about 10^4 x 6e-8 at worst; torch
    sums in blocks, so it stays far below)."""
    import torch
    g = kc.golden()
    out, lab, mask = _loss_cases()[case]
    loss = T.heatmap_loss_accuracy(out, lab, mask)[0]
    resid = torch.from_numpy(np.array(out)) * torch.from_numpy(np.array(mask)) - torch.from_numpy(np.array(lab))
    want = float(torch.nn.MSELoss()(resid.double(), torch.zeros_like(resid, dtype=torch.float64)))
    ref32 = float(g["a_%s_loss32" % case])
    print("loss %s: %.17g, float64 MSELoss %.17g (rel %.3g), reference float32 %.9g (rel %.3g)"
          % (case, loss, want, abs(loss - want) / want, ref32, abs(loss - ref32) / ref32))
    assert abs(loss - want) <= 1e-12 * want
    assert abs(loss - ref32) <= 1e-5 * ref32
    unmasked = T.heatmap_loss_accuracy(out, lab, None)[0]
    assert (unmasked == loss) == bool((np.array(mask) == 1).all())


@pytest.mark.parametrize("case", ["a", "b"])
def test_gradient_equals_autograd(case):
    """Bar: 4 ulps of the largest gradient magnitude (torch forms (2 / N) * residual * mask too; the orders of the two
    products may differ)."""
    import torch
    out, lab, mask = _loss_cases()[case]
    grad = T.heatmap_loss_accuracy(out, lab, mask, want_grad=True)[5]
    t = torch.tensor(np.array(out), requires_grad=True)
    torch.nn.MSELoss()(t * torch.from_numpy(np.array(mask)), torch.from_numpy(np.array(lab))).backward()
    want = t.grad.numpy()
    top = float(np.abs(want).max())
    worst = float(np.abs(grad - want).max()) / (EPS32 * top)
    print("gradient %s: worst %.3g ulp of the largest gradient %.3g" % (case, worst, top))
    assert top > 0 and worst <= 4
    assert T.heatmap_loss_accuracy(out, lab, mask)[5] is None


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_accuracy_equals_heatmapaccuracy(case):
    g = kc.golden()
    out, lab, mask = _loss_cases()[case]
    _, acc, preds, gt, dists, _ = T.heatmap_loss_accuracy(out, lab, mask)
    assert np.array_equal(preds, g["a_%s_preds" % case]) and np.array_equal(gt, g["a_%s_gt" % case])
    want = g["a_%s_dists" % case]
    assert np.array_equal(dists == -1, want == -1)
    assert ulps(dists, want)[want != -1].max(initial=0) <= 1
    assert np.array_equal(acc.view(np.uint32), g["a_%s_acc" % case].view(np.uint32))
    if case == "a":
        assert dists[2, 1] == -1 and (dists[5] == -1).all() and acc[6] == -1      # undrawn label; a channel nobody counts in
        assert preds[0, 0].tolist() == [7, 3]                                     # the tie goes to the lower flat index
        assert preds[2, 3].tolist() == [0, 0]                                     # a masked map
    if case == "b":
        assert dists[0, 0] == 0.5 and dists[0, 1] > 0.5 and acc[1] == 0.5         # 16 px^2 lands on the threshold and counts
    if case == "c":
        assert acc[0] == 0 and (acc[1:] == -1).all()


def test_draw_augmentation():
    d = T.draw_augmentation(np.random.default_rng(1), 4000)
    assert d["gains"].dtype == np.float32 and d["gains"].shape == (4000, 3) and 0.7 <= d["gains"].min() and d["gains"].max() <= 1.3
    assert 0.2 <= d["scale_rate"].min() and d["scale_rate"].max() <= 0.3
    assert 0.45 < d["flip"].mean() < 0.55 and 0.55 < (d["angle"] == 0).mean() < 0.65 and np.abs(d["angle"]).max() <= 80
    again = T.draw_augmentation(np.random.default_rng(1), 4000)
    assert all(np.array_equal(d[k], again[k]) for k in d)
    e = T.draw_augmentation(np.random.default_rng(1), 5, train=False)
    assert e["gains"] is None and not e["flip"].any() and not e["angle"].any() and e["scale_rate"].shape == (5,)


def test_argument_checks():
    fr = kc.frames_of(48, 64)
    ul, br = kc.window_cases(48, 64)
    with pytest.raises(ValueError):
        T.kpd_inputs(fr, [0, 2], ul[:2], br[:2])
    with pytest.raises(ValueError):
        T.kpd_inputs(fr, [0], ul[:2], br[:2])
    with pytest.raises(ValueError):
        T.kpd_inputs(fr.astype(np.float32), [0], ul[:1], br[:1])
    x = np.zeros((2, 3, 5, 4), np.float32)
    with pytest.raises(ValueError):
        T.augment_maps(x, [0], [0.0, 0.0])
    with pytest.raises(ValueError):
        T.augment_maps(x, [0, 0], [0.0, 0.0], ((1, 4),))
    with pytest.raises(ValueError):
        T.heatmap_loss_accuracy(x, x[:1])
    with pytest.raises(ValueError):
        A.kpd_targets(np.zeros((1, 2, 2)), ul[:1], br[:1], as_tensor=True)


def test_loader_host(tmp_path):
    annot = kc.write_folder(str(tmp_path))
    kw = dict(in_res=(20, 16), out_res=(10, 8))
    train = T.KPDSampleLoader(annot, str(tmp_path), 2, train=True, seed=4, **kw)
    batches = list(train)
    assert [b[0].shape for b in batches] == [(2, 3, 20, 16), (1, 3, 20, 16)] and len(train) == 2
    assert batches[0][1].shape == (2, 7, 10, 8) and (batches[0][2] == 1).all()
    again = list(T.KPDSampleLoader(annot, str(tmp_path), 2, train=True, seed=4, **kw))
    assert all(np.array_equal(a, b) for x, y in zip(batches, again) for a, b in zip(x, y))
    other = list(T.KPDSampleLoader(annot, str(tmp_path), 2, train=True, seed=5, **kw))
    assert not np.array_equal(other[0][0], batches[0][0])
    ev = T.KPDSampleLoader(annot, str(tmp_path), 3, train=False, seed=4, add_dpg=True, **kw)
    (inps, labels, mask), = list(ev)
    assert ev.last["ids"].tolist() == [0, 1, 2] and ev.last["gains"] is None
    # evaluation mode is the plain chain: windows -> targets / inputs, no augmentation
    from PIL import Image
    frames = np.stack([np.asarray(Image.open(os.path.join(str(tmp_path), "%012d.png" % i))) for i in range(3)])
    want = T.kpd_inputs(frames, [0, 1, 2], ev.last["ul"], ev.last["br"], None, ev.last["joint_num"] == 0, (20, 16))
    assert np.array_equal(inps, want) and inps.any()


def test_cli(tmp_path):
    annot = kc.write_folder(str(tmp_path))
    outs = [str(tmp_path / ("batch%d.npz" % i)) for i in range(2)]
    base = [sys.executable, os.path.join(ROOT, "kpd_samples.py"), "--annot", annot, "--img_folder", str(tmp_path), "--batch", "3",
            "--inputResH", "20", "--inputResW", "16", "--outputResH", "10", "--outputResW", "8"]
    for out in outs:
        r = subprocess.run(base + ["--seed", "7", "--addDPG", "--out", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    b = np.load(outs[0])
    assert sorted(b.files) == ["angle", "br", "flip", "gains", "ids", "inps", "joint_num", "labels", "scale_rate", "setMask", "ul"]
    assert b["inps"].shape == (3, 3, 20, 16) and b["labels"].shape == (3, 7, 10, 8) and b["setMask"].shape == (3, 7, 10, 8)
    assert b["ul"].shape == (3, 2) and b["gains"].shape == (3, 3) and sorted(b["ids"].tolist()) == [0, 1, 2]
    assert open(outs[0], "rb").read() == open(outs[1], "rb").read()
