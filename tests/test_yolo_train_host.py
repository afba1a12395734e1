"""The host twins of the detector-training calls (bp_yolo_inputs_host, bp_yolo_truth_host, bp_yolo_loss_host) against
tests/golden/yolo_train.npz, which the reference's own Darknet C code wrote (tools/make_golden_yolo_train.py).  No GPU.

The reference is compiled with -ffp-contract=fast -mfma and libm; the twins run with contraction off and their own
exp / log.  Every bar was measured on the CPU (the figure is printed before it is asserted) and is either derived or at
most 4 x the measured maximum:

  inputs, undistorted   bar 3.6e-7 absolute: six rounded float32 operations on values <= 1 (two products and a sum per
                        pass), 2^-24 each.  Measured 1.2e-7 (0 where only the crop or the flip acts).
  inputs, distorted     bar 2.2e-6 = 4 x the measured 5.4e-7 (the HSV round trip divides by max - min).
  truth rows            kept and the ids exact; boxes bar 4.8e-7 absolute = 4 x the measured 1.2e-7.  (The 1 ulp the
                        issue expected holds for the edges; w = right - left cancels, so its ulp count is larger.)
  loss, delta           the non-zero positions equal the reference's exactly; values bar 3.9e-6 absolute = 4 x the
                        measured 9.6e-7 (1 ulp of a box delta of magnitude 8 .. 16).
  loss, act             bar 6e-8 absolute: one float32 ulp below 1; measured 0.
  loss, cost            bar 1.6e-6 relative to the reference's float32 cost = 4 x the measured 3.9e-7 (the reference
                        sums squares in a float32 running sum; the twin in float64).
  loss, statistics      count exact; the rest against the six printed decimals: bar 2.6e-6 = 4 x the measured 6.4e-7, of
                        which up to 5e-7 is the printing (float32 running sums there, float64 here).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import yolo_train_common as yc

BAR_BILINEAR, BAR_DISTORT, BAR_TRUTH, BAR_DELTA, BAR_ACT, BAR_COST, BAR_STAT = 3.6e-7, 2.2e-6, 4.8e-7, 3.9e-6, 6e-8, 1.6e-6, 2.6e-6


def _iou(a, b):
    def ov(x1, w1, x2, w2):
        return np.minimum(x1 + w1 / 2, x2 + w2 / 2) - np.maximum(x1 - w1 / 2, x2 - w2 / 2)
    w, h = ov(a[..., 0], a[..., 2], b[..., 0], b[..., 2]), ov(a[..., 1], a[..., 3], b[..., 1], b[..., 3])
    inter = np.where((w < 0) | (h < 0), 0.0, w * h)
    return inter / (a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter)


def test_fixture_says_what_ran_and_its_conditions_hold():
    from betapose_amd import yolo_train as Y
    m, g = yc.meta(), yc.golden()
    assert m["exempt_cases"] == 0 and m["restated"]
    for name in ("crop_image", "resize_image", "flip_image", "distort_image", "fill_truth_detection", "forward_yolo_layer"):
        assert name in m["reference_ran"]
    assert os.path.getsize(os.path.join(yc.ROOT, "tests", "golden", "yolo_train.npz")) < 200 * 1024
    cond = m["conditions"]
    anchors = np.array(g["anchors"], np.float64)
    boxes9 = np.concatenate([np.zeros((9, 2)), anchors / yc.NET], 1)
    worst = dict(iou=1.0, anchor=1.0, cell=1.0, hue=1.0)
    names = set()
    for c in m["loss_cases"]:
        x, truth, kw, _, act = yc.loss_case(c)
        names.add((c["w"], c["h"], c["classes"], tuple(c["mask"]), c["ignore_thresh"], c["truth_thresh"]))
        B, _, h, w = act.shape
        a = act.reshape(B, 3, 5 + c["classes"], h, w).astype(np.float64)
        jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        an = anchors[c["mask"]]
        pred = np.stack([(ii + a[:, :, 0]) / w, (jj + a[:, :, 1]) / h, np.exp(a[:, :, 2]) * an[None, :, 0, None, None] / yc.NET,
                         np.exp(a[:, :, 3]) * an[None, :, 1, None, None] / yc.NET], -1)
        marks = np.array([c["ignore_thresh"], c["truth_thresh"], 0.5, 0.75])
        for b in range(B):
            rows = truth[b][:int(np.argmax(truth[b, :, 0] == 0)) if (truth[b, :, 0] == 0).any() else len(truth[b])].astype(np.float64)
            if not len(rows):
                continue
            best = _iou(pred[b][..., None, :], rows[:, :4]).max(-1)
            worst["iou"] = min(worst["iou"], float(np.abs(best[..., None] - marks).min()))
            for t in rows:
                s = np.sort(_iou(boxes9, np.array([0, 0, t[2], t[3]])))
                worst["anchor"] = min(worst["anchor"], float(s[-1] - s[-2]))
                fx, fy = t[0] * w, t[1] * h
                worst["cell"] = min(worst["cell"], abs(fx - round(fx)), abs(fy - round(fy)))
    for c in m["image_cases"]:
        if c["hsv"] is None:
            continue
        args, _ = yc.image_case(c)
        rgb = Y.yolo_inputs(*args[:4], None, args[5])[0].astype(np.float64)
        mx, mn = rgb.max(0), rgb.min(0)
        d = np.where(mx > mn, mx - mn, np.nan)
        r, gg, b = rgb
        hue = np.where(r == mx, (gg - b) / d, np.where(gg == mx, 2 + (b - r) / d, 4 + (r - gg) / d))
        hue = np.where(hue < 0, hue + 6, hue) / 6 + np.float32(c["hsv"][0])
        hue = hue[np.isfinite(hue)]
        worst["hue"] = min(worst["hue"], float(np.minimum(np.abs(hue), np.abs(hue - 1)).min()))
    print("condition gaps", worst)
    assert worst["iou"] > cond["iou_to_threshold"] and worst["anchor"] > cond["anchor_gap"]
    assert worst["cell"] > cond["cell_to_integer"] and worst["hue"] > cond["hue_to_wrap"]
    # the cases the issue names are all there
    assert {(n[0], n[1]) for n in names} == {(3, 2), (5, 7), (13, 13)} and {n[2] for n in names} == {1, 3}
    assert {n[3] for n in names} == {(0, 1, 2), (3, 4, 5), (6, 7, 8)}
    assert {n[4] for n in names} == {0.5, 0.7} and {n[5] for n in names} == {1.0, 0.9}
    assert all(c["cells_above_truth_thresh"] > 0 for c in m["loss_cases"] if c["truth_thresh"] < 1)
    assert {c["kept"] for c in m["truth_cases"]} >= {0, 1} and any(len(g["truth_%s_labels" % c["name"]]) == 95 for c in m["truth_cases"])


@pytest.mark.parametrize("case", [c["name"] for c in yc.meta()["image_cases"]])
def test_inputs_against_the_reference(case):
    from betapose_amd import yolo_train as Y
    c = [k for k in yc.meta()["image_cases"] if k["name"] == case][0]
    args, want = yc.image_case(c)
    got = Y.yolo_inputs(*args)
    err = float(np.abs(got - want).max())
    print("inputs", case, "max abs error", err)
    assert want.any() and got.shape == want.shape
    assert err <= (BAR_BILINEAR if c["hsv"] is None else BAR_DISTORT)
    if case in ("stage_crop", "stage_flip"):
        assert np.array_equal(got, want)        # no arithmetic but u8 / 255: exact


def test_inputs_zero_sample_and_batch_of_cases():
    from betapose_amd import yolo_train as Y
    cs = [c for c in yc.meta()["image_cases"] if c["frame"] == 1 and tuple(c["net"]) == (24, 16)]
    frames = np.array(yc.golden()["frame1"])[None]
    idx = np.array([0] * len(cs) + [1, -1], np.int32)
    crop = np.array([c["crop"] for c in cs] + [cs[0]["crop"]] * 2, np.int32)
    flip = np.array([c["flip"] for c in cs] + [0, 0], np.uint8)
    got = Y.yolo_inputs(frames, idx, crop, flip, None, (24, 16))
    assert not got[-2:].any()
    for k, c in enumerate(cs):
        if c["hsv"] is None:
            assert np.array_equal(got[k], Y.yolo_inputs(*yc.image_case(c)[0])[0])


@pytest.mark.parametrize("case", [c["name"] for c in yc.meta()["truth_cases"]])
def test_truth_against_the_reference(case):
    from betapose_amd import yolo_train as Y
    c = [k for k in yc.meta()["truth_cases"] if k["name"] == case][0]
    args, want = yc.truth_case(c)
    truth, kept = Y.yolo_truth(*args)
    err = float(np.abs(truth[..., :4] - want[..., :4]).max())
    print("truth", case, "kept", int(kept[0]), "max abs error", err)
    assert int(kept[0]) == c["kept"] == int((want[0, :, 0] != 0).sum())
    assert np.array_equal(truth[..., 4], want[..., 4]) and not truth[0, c["kept"]:].any()
    assert err <= BAR_TRUTH
    if case == "ninety_five_flip":      # cut to 90 rows first, then filtered: fewer than 90 are kept although 95 were read
        assert len(args[0]) == 95 and c["kept"] < 90
        assert c["kept"] == 90 - int((want[0, :, 0] == 0).sum()) and (want[0, :c["kept"], 0] != 0).all()


def test_truth_batch_equals_its_samples():
    from betapose_amd import yolo_train as Y
    args = yc.truth_batch()
    truth, kept = Y.yolo_truth(*args)
    for b, c in enumerate(yc.meta()["truth_cases"]):
        a1, _ = yc.truth_case(c)
        t1, k1 = Y.yolo_truth(*a1[:5], 3, *a1[6:])
        assert np.array_equal(t1[0], truth[b]) and k1[0] == kept[b]


@pytest.mark.parametrize("case", [c["name"] for c in yc.meta()["loss_cases"]])
def test_loss_against_the_reference(case):
    from betapose_amd import yolo_train as Y
    c = [k for k in yc.meta()["loss_cases"] if k["name"] == case][0]
    x, truth, kw, dwant, awant = yc.loss_case(c)
    cost, st, delta, act = Y.yolo_loss(x, truth, **kw)
    e_delta, e_act = float(np.abs(delta - dwant).max()), float(np.abs(act - awant).max())
    e_cost = abs(cost - c["cost"]) / c["cost"]
    want, count = yc.line_values(c["line"])
    cells = x.shape[0] * 3 * x.shape[2] * x.shape[3]
    mine = [st["iou"] / count, st["class"] / count, st["obj"] / count, st["anyobj"] / cells, st["recall50"] / count, st["recall75"] / count]
    e_stat = max(abs(a - b) for a, b in zip(mine, want))
    print("loss", case, "delta", e_delta, "act", e_act, "cost rel", e_cost, "stat", e_stat)
    assert dwant.any() and np.array_equal(delta != 0, dwant != 0)
    assert e_delta <= BAR_DELTA and e_act <= BAR_ACT and e_cost <= BAR_COST
    assert int(st["count"]) == count and count > 0 and e_stat <= BAR_STAT
    cost2, st2, delta2, _ = Y.yolo_loss(x, truth, want_act=False, **kw)
    assert cost2 == cost and st2 == st and np.array_equal(delta2, delta)


def test_loss_is_the_sum_of_squares_and_overwrites_in_order():
    from betapose_amd import yolo_train as Y
    c = [k for k in yc.meta()["loss_cases"] if k["name"] == "g5x7_c3_m0"][0]
    x, truth, kw, _, _ = yc.loss_case(c)
    cost, _, delta, _ = Y.yolo_loss(x, truth, **kw)
    assert abs(cost - float((delta.astype(np.float64) ** 2).sum())) <= 1e-12 * cost
    # two truths of one cell and anchor: the later row's box deltas stand, so swapping the rows changes them
    swapped = truth.copy()
    swapped[0, [3, 4]] = truth[0, [4, 3]]
    _, _, d2, _ = Y.yolo_loss(x, swapped, **kw)
    assert not np.array_equal(d2, delta)


def test_yolo_loss_backward_is_minus_delta():
    import torch
    from betapose_amd import yolo_train as Y
    c = [k for k in yc.meta()["loss_cases"] if k["name"] == "g3x2_c3_m1_t0"][0]
    x, truth, kw, _, _ = yc.loss_case(c)
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(4, x.shape[1], 1)
    inp = torch.randn(x.shape[0], 4, x.shape[2], x.shape[3])
    out = conv(inp)
    loss = Y.YoloLoss.apply(out, torch.from_numpy(truth), kw["net_size"], kw["anchors"], kw["mask"], kw["classes"], kw["ignore_thresh"],
                            kw["truth_thresh"])
    cost, _, delta, _ = Y.yolo_loss(out.detach().numpy(), truth, **kw)
    assert float(loss.detach()) == pytest.approx(cost, rel=1e-6)
    (3 * loss).backward()
    g_w, g_b = conv.weight.grad.clone(), conv.bias.grad.clone()
    conv.zero_grad()
    conv(inp).backward(torch.from_numpy(-3 * delta))    # what -delta * grad_output hands to the layer below
    assert g_w.abs().max() > 0 and torch.equal(conv.weight.grad, g_w) and torch.equal(conv.bias.grad, g_b)
    assert np.array_equal(Y.YoloLoss.last["delta"].numpy(), delta)


def test_samples_cli_writes_the_loaders_batch(tmp_path):
    from betapose_amd import yolo_train as Y
    lst = yc.write_folder(str(tmp_path / "set"))
    out = str(tmp_path / "batch.npz")
    r = subprocess.run([sys.executable, os.path.join(yc.ROOT, "yolo_samples.py"), "--list", lst, "--batch", "2", "--seed", "4", "--width", "32",
                        "--height", "24", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    z = np.load(out)
    from betapose_amd.cfg import parse_cfg
    blocks = parse_cfg("yolov3-single.cfg")
    net = blocks[0] if blocks[0].get("type") == "net" else {}
    yolo = [b for b in blocks if b.get("type") == "yolo"][0]
    loader = Y.YoloSampleLoader(lst, 2, net_size=(24, 32), classes=Y.yolo_head_params(blocks)[0]["classes"], seed=4,
                                jitter=float(yolo.get("jitter", .2)), hue=float(net.get("hue", 0)),
                                saturation=float(net.get("saturation", 1)), exposure=float(net.get("exposure", 1)))
    batches = list(loader)
    assert len(batches) == 2 and batches[1][0].shape[0] == 1
    loader.epoch = 0
    inps, truth = next(iter(loader))
    assert np.array_equal(z["inps"], inps) and np.array_equal(z["truth"], truth) and z["inps"].shape == (2, 3, 24, 32)
    assert np.array_equal(z["kept"], loader.last["kept"]) and (z["kept"] > 0).all() and inps.any()
    # evaluation mode: whole frames in order, nothing drawn
    ev = Y.YoloSampleLoader(lst, 3, net_size=(48, 64), train=False)
    e_inps, e_truth = next(iter(ev))
    from PIL import Image
    first = np.asarray(Image.open(open(lst).read().split()[0]))
    assert np.array_equal(e_inps[0], (first.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    assert np.array_equal(ev.last["kept"], [1, 2, 3])


def test_draws_labels_and_head_parameters(tmp_path):
    from betapose_amd import yolo_train as Y
    from betapose_amd.cfg import parse_cfg_text
    crop, geom, flip, hsv = Y.draw_detection_augmentation(np.random.default_rng(1), 500, (480, 640))
    dw, dh = int(640 * 0.3), int(480 * 0.3)
    assert crop.dtype == np.int32 and (np.abs(crop[:, 0]) <= dw).all() and (np.abs(crop[:, 1]) <= dh).all()
    assert (crop[:, 2] >= 640 - 2 * dw).all() and (crop[:, 2] <= 640 + 2 * dw).all() and set(flip) == {0, 1}
    assert np.allclose(geom[:, 2], 640 / crop[:, 2], rtol=1e-6) and np.allclose(geom[:, 0], crop[:, 0] / crop[:, 2], atol=1e-6)
    assert (np.abs(hsv[:, 0]) <= 0.3).all() and (hsv[:, 1:] >= 1 / 1.5 - 1e-6).all() and (hsv[:, 1:] <= 1.5).all()
    assert (hsv[:, 1] < 1).any() and (hsv[:, 1] > 1).any()
    assert Y.label_path("/d/JPEGImages/a.jpg ") == "/d/labels/a.txt" and Y.label_path("/d/images/train2014/b.PNG") == "/d/labels/train2014/b.txt"
    assert Y.label_path("/d/a.jpg.jpg") == "/d/a.jpg.jpg"       # the first occurrence of the extension is not the end: kept
    p = tmp_path / "l.txt"
    p.write_text("0 0.5 0.25 0.1 0.2\n2 0.1 0.2 0.3 0.4\nx\n")
    labels, first = Y.read_labels([str(p), str(tmp_path / "missing.txt")])
    assert labels.tolist() == np.array([[0, .5, .25, .1, .2], [2, .1, .2, .3, .4]], np.float32).tolist() and first.tolist() == [0, 2, 2]
    heads = Y.yolo_head_params(parse_cfg_text("[net]\nwidth=416\n[yolo]\nmask = 3,4,5\nanchors = 1,2, 3,4, 5,6, 7,8, 9,10, 11,12\n"
                                              "classes=2\nnum=6\nignore_thresh = .7\n"))
    assert len(heads) == 1 and heads[0]["mask"].tolist() == [3, 4, 5] and heads[0]["anchors"].shape == (6, 2)
    assert heads[0]["classes"] == 2 and heads[0]["ignore_thresh"] == 0.7 and heads[0]["truth_thresh"] == 1.0


def test_argument_errors_return_an_error_code():
    from betapose_amd import _lib
    L = _lib.lib()
    f = np.zeros((1, 8, 8, 3), np.uint8)
    idx, flip, out = np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros((1, 3, 4, 4), np.float32)
    call = lambda crop, nh=4, nw=4: L.bp_yolo_inputs_host(_lib.ptr(f), 1, 8, 8, _lib.ptr(idx), _lib.ptr(np.array(crop, np.int32)),
                                                         _lib.ptr(flip), None, 1, nh, nw, _lib.ptr(out))
    assert call([0, 0, 8, 8]) == 0
    assert call([0, 0, 1, 8]) != 0 and call([0, 0, 8, 1]) != 0 and call([0, 0, 8, 8], 1, 4) != 0 and call([0, 0, 8, 8], 4, 1) != 0
    assert b"swidth" in L.bp_last_error() or call([0, 0, 1, 8]) != 0
    x = np.zeros((1, 18, 2, 2), np.float32)
    anchors, mask = np.ones((9, 2), np.float32), np.array([0, 1, 2], np.int32)
    truth, delta = np.zeros((1, 90, 5), np.float32), np.zeros_like(x)
    cost, stats, partial = np.zeros(1), np.zeros(7), np.zeros(64)
    loss = lambda channels=18, classes=1, focal=0, m=mask: L.bp_yolo_loss_host(
        _lib.ptr(x), 1, channels, 3, classes, 2, 2, 416, 416, _lib.ptr(anchors), 9, _lib.ptr(m), _lib.ptr(truth), 90, 0.7, 1.0, focal, None,
        _lib.ptr(delta), _lib.ptr(cost), _lib.ptr(stats), _lib.ptr(partial))
    assert loss() == 0
    assert loss(focal=1) != 0 and loss(classes=2) != 0 and loss(channels=21) != 0 and loss(m=np.array([0, 1, 9], np.int32)) != 0
    with pytest.raises(_lib.BetaposeHipError):
        from betapose_amd import yolo_train as Y
        Y.yolo_loss(x, truth, (416, 416), anchors, mask, classes=2)
