"""Detector validation on the GPU: every output of bp_yolo_detections, bp_detector_map_match and bp_detector_map_reduce
has the bits of its host twin, on the reference's cases and on seeded ones, at several batch sizes, on a second stream
and twice in a row."""
import numpy as np
import pytest

import yolo_map_common as C
from betapose_amd import yolo_map as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _chain(pred, heads, net, classes, labels, first, nms=.45, max_dets=256, device=None):
    """calls 1 to 3 on one batch: every output as numpy arrays"""
    dets, count, over = M.yolo_detections(pred, heads, net, classes, .005, nms, max_dets, device)
    m = M.map_match(dets, count, labels, first, classes, .5, .25, 7, 3, None, None, device)
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    rc = host(m["rec_count"])
    rec = host(m["rec"])
    flat = np.concatenate([rec[b, :rc[b]] for b in range(len(rc))]) if len(rc) else rec.reshape(-1, 6)
    r = M.map_reduce(flat if device is None else __import__("torch").from_numpy(flat).to(device), m["truth_classes_count"],
                     7 + len(labels), m["img_stats"], classes, True, device)
    out = dict(dets=dets, count=count, rec=m["rec"], rec_count=m["rec_count"], tcc=m["truth_classes_count"], img_stats=m["img_stats"],
               ap=r["ap"], stats=r["stats"], pr=r["pr"])
    return {k: host(v) for k, v in out.items()}, over


def _same(a, b):
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("case", C.meta()["a_cases"], ids=lambda c: c["name"])
def test_box_list_cases_bit_equal(case):
    pred, heads, net, classes, nms = C.a_case(case)
    labels, first = np.zeros((0, 5), np.float32), np.zeros(2, np.int32)
    md = min(pred.shape[1], 4096)
    h, _ = _chain(pred, heads, net, classes, labels, first, nms, md)
    d, _ = _chain(pred, heads, net, classes, labels, first, nms, md, DEV)
    _same(h, d)


@pytest.mark.parametrize("case", C.meta()["b_cases"], ids=lambda c: c["name"])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_accounting_cases_bit_equal(case, B):
    pred, labels, first, heads, net, classes = C.b_case(case)
    lab, fr = labels[first[2]:first[2 + B]], (first[2:3 + B] - first[2]).astype(np.int32)
    h, _ = _chain(pred[2:2 + B], heads, net, classes, lab, fr)
    d, _ = _chain(pred[2:2 + B], heads, net, classes, lab, fr, device=DEV)
    _same(h, d)


@pytest.mark.parametrize("counts,classes,max_dets", [((0, 1, 63, 64, 65), 1, 128), ((1023, 1025, 1024), 3, 1024), ((1025, 7), 1, 1024),
                                                     ((300, 0, 17), 16, 512)])
def test_candidate_counts_bit_equal(counts, classes, max_dets):
    import torch
    pred, heads = C.seeded_pred(5, counts, classes)
    labels, first = C.seeded_labels(5, pred, classes)
    h, ho = _chain(pred, heads, C.SEED_NET, classes, labels, first, max_dets=max_dets)
    d, do = _chain(pred, heads, C.SEED_NET, classes, labels, first, max_dets=max_dets, device=DEV)
    _same(h, d)
    assert list(d["count"]) == list(counts)
    assert sorted(do) == sorted(ho) == [b for b, c in enumerate(counts) if c > max_dets]     # overflow is reported
    for b in do:
        assert not d["dets"][b].any() and np.array_equal(do[b], ho[b]) and len(do[b]) == counts[b]
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        s, _ = _chain(pred, heads, C.SEED_NET, classes, labels, first, max_dets=max_dets, device=DEV)
    side.synchronize()
    _same(d, s)
    again, _ = _chain(pred, heads, C.SEED_NET, classes, labels, first, max_dets=max_dets, device=DEV)
    _same(d, again)


def test_device_cap_exactly_and_one_more():
    cap = M.max_dets_cap()
    assert cap == 4096
    big = [(3, 37, 37)]                                                 # 4 107 rows
    pred, heads = C.seeded_pred(6, (cap, cap + 1), 1, heads=big)
    labels, first = C.seeded_labels(6, pred, 1)
    h, ho = _chain(pred, heads, C.SEED_NET, 1, labels, first, max_dets=cap)
    d, do = _chain(pred, heads, C.SEED_NET, 1, labels, first, max_dets=cap, device=DEV)
    _same(h, d)
    assert list(d["count"]) == [cap, cap + 1] and d["dets"][0, cap - 1].any() and not d["dets"][1].any()
    assert list(do) == list(ho) == [1] and np.array_equal(do[1], ho[1])


@pytest.mark.parametrize("D,classes", [(0, 3), (1, 1), (2049, 3), (5000, 16)])
def test_reduce_sizes_bit_equal(D, classes):
    rec, tcc, st = C.seeded_records(9, D, classes, 40)
    h = M.map_reduce(rec, tcc, 40, st, classes, True)
    d = M.map_reduce(rec, tcc, 40, st, classes, True, DEV)
    for k in ("ap", "stats", "pr"):
        assert h[k].tobytes() == d[k].cpu().numpy().tobytes(), k


def test_detector_map_object_on_device():
    case = C.meta()["b_cases"][1]
    pred, labels, first, heads, net, classes = C.b_case(case)
    res = []
    counts = M.yolo_detections(pred, heads, net, classes, max_dets=pred.shape[1])[1]
    cut = int(np.median(counts))                                        # the frames above the median overflow and are redone
    for dev in (None, DEV):
        dm = M.DetectorMap(classes, heads, net, max_dets=cut, device=dev)
        for s in range(0, len(pred), 5):
            e = min(s + 5, len(pred))
            dm.update(pred[s:e], labels[first[s]:first[e]], (first[s:e + 1] - first[s]).astype(np.int32))
        res.append(dm.result())
    a, b = res
    rep = case["report"]
    assert np.array_equal(a["ap"], b["ap"]) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in M.STAT_NAMES)
    assert a["overflow_images"] == b["overflow_images"] and len(a["overflow_images"]) > 0
    assert (b["detections_count"], b["tp"], b["fp"], b["fn"]) == (rep["detections_count"], rep["tp"], rep["fp"], rep["fn"])


@pytest.mark.parametrize("case", C.meta()["b_cases"], ids=lambda c: c["name"])
def test_end_to_end_through_the_engine(case, tmp_path):
    """detector_map.py's function on the reference's validation tree: frames, the resize_image input path, the engine of
    bp_yolo_create_darknet in bf16x3 mode and the tail, against validate_detector_map's own report.  The generator's
    margins (1e-4 in IoU, 1e-6 in prob) are what makes the counts robust to the engine's rounding."""
    import os
    import sys
    sys.path.insert(0, C.ROOT)
    import detector_map
    root = str(tmp_path / "tree")
    data = C.write_b_tree(case, root)
    r, names = detector_map.detector_map(data, os.path.join(root, "net.cfg"), os.path.join(root, "net.weights"), .25, .5, batch=5,
                                         device=DEV, max_dets=256)
    rep = case["report"]
    print(r["detections_count"], rep["detections_count"], r["ap"] * 100, rep["ap"], r["tp"], r["fp"], r["fn"], r["mAP"], rep["mAP"])
    assert names == ["obj%d" % k for k in range(case["classes"])]
    assert (r["detections_count"], r["unique_truth_count"]) == (rep["detections_count"], rep["unique_truth_count"])
    assert (r["tp"], r["fp"], r["fn"]) == (rep["tp"], rep["fp"], rep["fn"])
    assert np.abs(r["ap"] * 100 - np.array(rep["ap"])).max() <= 0.005 + 1e-9
    assert abs(r["avg_iou"] * 100 - rep["avg_iou"]) <= 0.005 + 1e-9 and abs(r["mAP"] - rep["mAP"]) <= 5e-7 + 1e-12
    for k in ("precision", "recall", "f1"):
        assert abs(r[k] - rep[k]) <= 0.005 + 1e-9


def test_data_file_with_difficult_is_refused(tmp_path):
    import os
    import sys
    sys.path.insert(0, C.ROOT)
    import detector_map
    case = C.meta()["b_cases"][0]
    root = str(tmp_path / "tree")
    data = C.write_b_tree(case, root)
    with open(data, "a") as f:
        f.write("difficult = %s\n" % os.path.join(root, "valid.txt"))
    with pytest.raises(ValueError, match="difficult"):
        detector_map.detector_map(data, os.path.join(root, "net.cfg"), os.path.join(root, "net.weights"), device=DEV)
