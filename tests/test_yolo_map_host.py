"""Detector validation on the host twins (no GPU): the box list against the reference's get_network_boxes + do_nms_sort,
the accounting against validate_detector_map's own report (tests/golden/yolo_map.npz, tools/make_golden_yolo_map.py),
properties on seeded inputs, and the helpers of detector_map.py."""
import numpy as np
import pytest

import yolo_map_common as C
from betapose_amd import yolo_map as M

# Boxes and probs against the reference, as |got - ref| / max(1, |ref|): measured maximum 1.19e-7 over every group A case
# (one float32 ulp: x / net_w against (i + x) / lw; the 64-pixel cases have box sizes up to 4, where an ulp is 2.4e-7
# absolute); the bound is twice that
BOX_TOL = 2.4e-7


@pytest.mark.parametrize("case", C.meta()["a_cases"], ids=lambda c: c["name"])
def test_box_list_against_reference(case):
    g = C.golden()
    pred, heads, net, classes, nms = C.a_case(case)
    dets, count, over = M.yolo_detections(pred, heads, net, classes, .005, nms, max_dets=pred.shape[1])
    n = int(count[0])
    index, live, ref = np.array(g["a_%s_index" % case["name"]]), np.array(g["a_%s_live" % case["name"]]), np.array(g["a_%s_dets" % case["name"]])
    assert n == case["candidates"] == len(index) and not over
    d = dets[0, :n]
    cand = d[:, 5].view(np.int32)                                       # Darknet's index over all rows; the archive counts candidates
    assert len(np.unique(cand)) == n and (cand >= 0).all() and (cand < pred.shape[1]).all()
    assert np.array_equal(np.argsort(np.argsort(cand)), index)          # every entry, in the reference's order
    assert np.array_equal(np.nonzero((d[:, 6:] > 0).any(1))[0], live)   # the same survivors
    assert np.array_equal(d[live][:, 6:] > 0, ref[:, 5:] > 0)
    got = np.concatenate([d[live][:, :5], d[live][:, 6:]], 1)
    err = float((np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max()) if len(ref) else 0.0
    print("max abs error", err)
    assert err <= BOX_TOL
    assert not dets[0, n:].any()


@pytest.mark.parametrize("case", C.meta()["b_cases"], ids=lambda c: c["name"])
def test_accounting_against_reference(case):
    pred, labels, first, heads, net, classes = C.b_case(case)
    rep = case["report"]
    for order in (range(len(pred)), reversed(range(len(pred)))):       # one image per update, in both orders
        dm = M.DetectorMap(classes, heads, net, max_dets=pred.shape[1])
        for f in order:                                                 # the reference numbers images and truths in list order
            dm.update(pred[f:f + 1], labels[first[f]:first[f + 1]], np.array([0, first[f + 1] - first[f]], np.int32), image_base=f,
                      truth_base=int(first[f]))
        r = dm.result()
        assert (r["detections_count"], r["unique_truth_count"]) == (rep["detections_count"], rep["unique_truth_count"])
        assert (r["tp"], r["fp"], r["fn"]) == (rep["tp"], rep["fp"], rep["fn"])
        assert list(r["truth_classes_count"]) == case["truth_classes_count"]
        print(r["ap"] * 100, rep["ap"], r["mAP"], rep["mAP"], r["avg_iou"] * 100, rep["avg_iou"])
        assert np.abs(r["ap"] * 100 - np.array(rep["ap"])).max() <= 0.005 + 1e-9
        assert abs(r["avg_iou"] * 100 - rep["avg_iou"]) <= 0.005 + 1e-9
        assert abs(r["mAP"] - rep["mAP"]) <= 5e-7 + 1e-12
        for k in ("precision", "recall", "f1"):
            assert abs(r[k] - rep[k]) <= 0.005 + 1e-9
    whole = M.DetectorMap(classes, heads, net, max_dets=pred.shape[1])   # the whole list as one batch
    whole.update(pred, labels, first)
    w = whole.result()
    assert np.array_equal(w["ap"], r["ap"]) and w["mAP"] == r["mAP"] and (w["tp"], w["fp"]) == (r["tp"], r["fp"])


def test_ten_truths_point_three():
    """10 truths, 3 found: recall 3 / 10 is below 3 * 0.1 in double, so the point at 0.3 takes no precision from it"""
    rec = np.zeros((3, 6), np.float32)
    rec[:, 0] = (.9, .8, .7)
    rec[:, 3] = np.arange(3, dtype=np.int32).view(np.float32)
    rec[:, 5] = np.arange(3, dtype=np.int32).view(np.float32)
    r = M.map_reduce(rec, np.array([10], np.int32), 10, np.zeros((1, 3)), 1)
    assert r["ap"][0] == 3.0 / 11 and (3 / 10 >= 3 * 0.1) is False


def _perfect(classes, images=3, per=4, seed=1):
    rng = np.random.default_rng(seed)
    heads = C.table([(1, 4, 4)])
    pred = np.zeros((images, 16, 5 + classes), np.float32)
    rows, first = [], [0]
    for b in range(images):
        for j, cell in enumerate(rng.permutation(16)[:per]):
            k = j % classes
            box = ((cell % 4) * 16 + 8, (cell // 4) * 16 + 8, 12, 10)
            pred[b, cell, :4], pred[b, cell, 4], pred[b, cell, 5 + k] = box, 0.9 - 0.01 * j - 0.1 * b, 1.0
            rows.append((k,) + tuple(v / 64 for v in box))
        first.append(len(rows))
    return pred, np.array(rows, np.float32), np.array(first, np.int32), heads


@pytest.mark.parametrize("classes", [1, 3])
def test_perfect_detector(classes):
    pred, labels, first, heads = _perfect(classes)
    dm = M.DetectorMap(classes, heads, (64, 64))
    dm.update(pred, labels, first)
    r = dm.result()
    assert np.array_equal(r["ap"], np.ones(classes)) and r["mAP"] == 1.0
    assert (r["tp"], r["fp"], r["fn"]) == (len(labels), 0, 0) and r["precision"] == r["recall"] == r["f1"] == 1.0


def test_no_detections_and_class_without_truths():
    pred, labels, first, heads = _perfect(3)
    dm = M.DetectorMap(3, heads, (64, 64))
    dm.update(np.zeros_like(pred), labels, first)
    r = dm.result()
    assert not r["ap"].any() and r["mAP"] == 0.0 and r["detections_count"] == 0 and (r["tp"], r["fp"], r["fn"]) == (0, 0, len(labels))
    labels0 = labels[labels[:, 0] != 2]                                 # class 2 keeps its detections and loses its truths
    first0 = np.searchsorted(np.nonzero(labels[:, 0] != 2)[0], first).astype(np.int32)
    dm = M.DetectorMap(3, heads, (64, 64))
    dm.update(pred, labels0, first0)
    r = dm.result()
    assert r["ap"][2] == 0.0 and r["ap"][0] == r["ap"][1] == 1.0 and r["fp"] == int((labels[:, 0] == 2).sum())


def test_overflow_is_reported_and_redone():
    pred, heads = C.seeded_pred(3, (40, 9, 33), 3)
    labels, first = C.seeded_labels(3, pred, 3)
    full = M.DetectorMap(3, heads, C.SEED_NET, max_dets=64)
    full.update(pred, labels, first)
    cut = M.DetectorMap(3, heads, C.SEED_NET, max_dets=32)
    dets, count = cut.update(pred, labels, first)
    assert list(count) == [40, 9, 33] and not dets[0].any() and not dets[2].any()
    a, b = full.result(), cut.result()
    assert b["overflow_images"] == [0, 2] and a["overflow_images"] == []
    assert np.array_equal(a["ap"], b["ap"]) and all(a[k] == b[k] for k in M.STAT_NAMES) and a["detections_count"] == b["detections_count"]


def test_reduce_matches_plain_statement():
    for D, classes, truths in ((0, 2, 5), (1, 1, 1), (700, 3, 60)):
        rec, tcc, st = C.seeded_records(11, D, classes, truths)
        r = M.map_reduce(rec, tcc, truths, st, classes, want_pr=True)
        ap, s = C.reduce_plain(rec, tcc, classes, truths, st)
        assert np.array_equal(r["ap"], ap) and r["stats"][0] == s["mAP"] and (r["stats"][5], r["stats"][6]) == (s["tp"], s["fp"])
        assert r["pr"].shape == (classes, D, 2)


def test_cli_helpers(tmp_path, capsys):
    case = C.meta()["b_cases"][0]
    data = C.write_b_tree(case, str(tmp_path / "tree"))
    opts = M.read_data_cfg(data)
    assert opts["classes"] == case["classes"] and opts["valid"].endswith("valid.txt") and opts["names"].endswith("obj.names")
    pred, labels, first, heads, net, classes = C.b_case(case)
    dm = M.DetectorMap(classes, heads, net, max_dets=pred.shape[1])
    dm.update(pred, labels, first)
    lines = M.report_lines(dm.result(), ["obj0"])
    rep = case["report"]
    assert lines[0].startswith("detections_count = %d, unique_truth_count = %d" % (rep["detections_count"], rep["unique_truth_count"]))
    assert lines[1].startswith("class_id = 0, name = obj0, \t ap = ") and lines[1].endswith(" % ")
    assert "TP = %d, FP = %d, FN = %d" % (rep["tp"], rep["fp"], rep["fn"]) in lines[3]
    assert lines[-1].startswith(" mean average precision (mAP) = ")
