"""ADD-S on the host (metrics.add_s_err), the symmetric option of evaluate_results and the --symmetric_ids flag: no GPU."""
import numpy as np

from betapose_amd import metrics
from betapose_amd.opt import build_parser, id_list


def rand_pose(rng, z=(0.6, 1.2)):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, zq = q
    R = np.array([[1 - 2 * (y * y + zq * zq), 2 * (x * y - zq * w), 2 * (x * zq + y * w)],
                  [2 * (x * y + zq * w), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - x * w)],
                  [2 * (x * zq - y * w), 2 * (y * zq + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(*z)]
    return T


def perturb(rng, T, rot=0.05, trans=0.01):
    a = rng.normal(size=3) * rot
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.linalg.norm(a)
    dR = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    E = T.copy()
    E[:3, :3] = T[:3, :3] @ dR
    E[:3, 3] = T[:3, 3] + rng.normal(size=3) * trans
    return E


def rz(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    return T


def test_add_s_zero_for_identical_pose():
    rng = np.random.default_rng(1)
    model = rng.normal(size=(500, 3)) * 0.05
    T = rand_pose(rng)
    assert metrics.add_s_err(T, T, model) == 0.0


def test_add_s_never_above_add():
    rng = np.random.default_rng(2)
    model = rng.normal(size=(700, 3)) * 0.05
    for _ in range(10):
        g = rand_pose(rng)
        e = perturb(rng, g)
        assert metrics.add_s_err(g, e, model) <= metrics.add_err(g, e, model) + 1e-15


def test_add_s_forgives_a_symmetry_turn():
    """A model made of point pairs exchanged by a 180-degree turn about z: the turned pose is a perfect ADD-S match and
    a plain-ADD miss."""
    rng = np.random.default_rng(3)
    half = rng.normal(size=(400, 3)) * 0.05
    model = np.concatenate([half, half * [-1, -1, 1]])
    g = rand_pose(rng)
    e = g @ rz(180)
    assert metrics.add_s_err(g, e, model) < 1e-12
    assert metrics.add_err(g, e, model) > 1e-3


def test_add_s_matches_kdtree_nearest_neighbours():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(4)
    model = rng.normal(size=(3000, 3)) * [0.04, 0.03, 0.02]
    for _ in range(5):
        g = rand_pose(rng)
        e = perturb(rng, g)
        a = model @ g[:3, :3].T + g[:3, 3]
        b = model @ e[:3, :3].T + e[:3, 3]
        d, _ = cKDTree(b).query(a, k=1)
        assert abs(metrics.add_s_err(g, e, model) - float(np.mean(d))) < 1e-12


def test_pose_errors_host_columns():
    rng = np.random.default_rng(5)
    model = rng.normal(size=(200, 3)) * 0.05
    cam = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]])
    gts = [rand_pose(rng) for _ in range(3)]
    ests = [perturb(rng, g) for g in gts]
    add, adds, proj = metrics.pose_errors(np.stack(gts), np.stack(ests)[:, :3], model, cam)
    for p in range(3):
        assert add[p] == metrics.add_err(gts[p], ests[p], model)
        assert adds[p] == metrics.add_s_err(gts[p], ests[p], model)
        assert proj[p] == metrics.projection_error_2d(gts[p], ests[p], model, cam)


def _evaluate_results_before(final_result, gt_frames, model_vertices, cam_K, diameter_mm, pixel_thresh=5.0):
    """evaluate_results as it was before the symmetric option (the yardstick of the default path)."""
    import os
    add_errs, adds, proj, ious = [], [], [], []
    for f in final_result:
        nr = int(os.path.basename(f["imgname"])[0:-4])
        if nr not in gt_frames:
            continue
        entries = gt_frames[nr]
        if isinstance(entries, dict):
            entries = [entries]
        for gt in entries:
            if len(f["result"]) < 1 or len(f["result"][0]) < 1:
                continue
            x, y, w, h = gt["bbox"]
            i = metrics.iou([x, y, x + w, y + h], np.asarray(f["result"][0]["bbox"]).tolist())
            ious.append(i)
            pose = np.eye(4)
            pose[:3, :3] = f["cam_R"]
            pose[:3, 3] = np.asarray(f["cam_t"])[:, 0]
            if i >= 0.5:
                a = metrics.add_err(gt["pose"], pose, model_vertices) * 1000
                add_errs.append(a)
                adds.append(a < diameter_mm / 10)
                proj.append(metrics.projection_error_2d(gt["pose"], pose, model_vertices, cam_K))
    return {"mean_add": float(np.mean(adds)) if adds else float("nan"),
            "mean_2d_acc": float(np.mean(np.array(proj) < pixel_thresh)) if proj else float("nan"),
            "mean_iou": float(np.mean(np.array(ious) > 0.5)) if ious else float("nan"),
            "mean_add_err_mm": float(np.mean(add_errs)) if add_errs else float("nan"), "n": len(ious)}


def synthetic_run(seed=6, frames=12, sym_model=False):
    """(final_result, gt_frames, model, cam): estimates near the ground truth, some boxes off (IoU < 0.5), some
    estimates turned by 180 degrees about z."""
    rng = np.random.default_rng(seed)
    half = rng.normal(size=(150, 3)) * 0.04
    model = np.concatenate([half, half * [-1, -1, 1]]) if sym_model else rng.normal(size=(300, 3)) * 0.04
    cam = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]])
    final_result, gt_frames = [], {}
    for nr in range(frames):
        g = rand_pose(rng)
        e = perturb(rng, g, rot=0.03, trans=0.006)
        if nr % 3 == 1:
            e = e @ rz(180)
        box = [100.0 + nr, 80.0, 80.0, 90.0]
        off = 60.0 if nr % 5 == 4 else 2.0
        gt_frames[nr] = [{"pose": g, "bbox": box}]
        final_result.append({"imgname": "%04d.png" % nr,
                             "result": [{"bbox": [box[0] + off, box[1], box[0] + box[2] + off, box[1] + box[3]]}],
                             "cam_R": e[:3, :3], "cam_t": e[:3, 3:4]})
    return final_result, gt_frames, model, cam


def test_evaluate_results_default_unchanged_and_symmetric_keys():
    fr, gtf, model, cam = synthetic_run()
    before = _evaluate_results_before(fr, gtf, model, cam, 100.0)
    now = metrics.evaluate_results(fr, gtf, model, cam, 100.0)
    assert now == before
    sym = metrics.evaluate_results(fr, gtf, model, cam, 100.0, symmetric=True)
    assert set(sym) - set(now) == {"mean_adds", "mean_adds_err_mm"}
    assert {k: sym[k] for k in now} == now
    assert sym["mean_adds_err_mm"] <= sym["mean_add_err_mm"]


def test_evaluate_results_symmetric_scores_turned_estimates():
    fr, gtf, model, cam = synthetic_run(sym_model=True)
    m = metrics.evaluate_results(fr, gtf, model, cam, 100.0, symmetric=True)
    assert m["mean_adds"] > m["mean_add"]


def test_symmetric_ids_flag():
    assert build_parser().parse_args([]).symmetric_ids == ""
    ns = build_parser().parse_args(["--symmetric_ids", "10,11"])
    assert id_list(ns.symmetric_ids) == [10, 11]
    assert id_list("") == []
    assert "10" in build_parser().format_help() and "11" in build_parser().format_help()
