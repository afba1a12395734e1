"""The BOP symmetry-aware errors on the host: metrics.symmetry_transforms / load_symmetries, mssd_err / mspd_err, the
average recalls of evaluate_results(symmetries=...), write_sixd_tree(symmetries=...) and the --bop_metrics flag: no GPU."""
import os

import numpy as np
import pytest

from betapose_amd import metrics, synth
from betapose_amd.opt import build_parser

CAM = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
HALF_TURN_Z = [-1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]
N_CONT = 315          # ceil(pi / 0.01)


def rand_rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rand_pose(rng):
    T = np.eye(4)
    T[:3, :3] = rand_rot(rng)
    T[:3, 3] = [rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)]
    return T


def perturb(rng, T, rot=0.05, trans=0.01):
    a = rng.normal(size=3) * rot
    th = np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / th
    E = T.copy()
    E[:3, :3] = T[:3, :3] @ (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)
    E[:3, 3] = T[:3, 3] + rng.normal(size=3) * trans
    return E


def rot_about(axis, th):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * A + (1 - np.cos(th)) * A @ A


def rz44(phi):
    T = np.eye(4)
    T[:3, :3] = rot_about([0, 0, 1], phi)
    return T


IDENTITY = np.eye(4)[None, :3, :]


# ---------------------------------------------------------------------------------------------- symmetry_transforms

def test_no_fields_is_identity():
    for entry in ({}, {"diameter": 100.0}, None):
        s = metrics.symmetry_transforms(entry)
        assert s.shape == (1, 3, 4) and s.dtype == np.float64
        assert np.array_equal(s[0], np.eye(4)[:3])


def test_one_discrete_half_turn():
    s = metrics.symmetry_transforms({"symmetries_discrete": [HALF_TURN_Z]})
    assert s.shape == (2, 3, 4)
    assert np.array_equal(s[0], np.eye(4)[:3])
    assert np.array_equal(s[1], np.diag([-1.0, -1.0, 1.0, 1.0])[:3])


def test_one_continuous_axis():
    axis, offset_mm = [1.0, 2.0, -2.0], [10.0, -20.0, 30.0]
    s = metrics.symmetry_transforms({"symmetries_continuous": [{"axis": axis, "offset": offset_mm}]})
    assert s.shape == (N_CONT, 3, 4)
    assert np.abs(s[0] - np.eye(4)[:3]).max() == 0.0
    off = np.array(offset_mm) / 1000.0
    for i in (1, 2, 157, 158, 314):
        assert np.abs(s[i][:, :3] - rot_about(axis, i * 2 * np.pi / N_CONT)).max() < 1e-15
    # the offset is a fixed point of every element, and so is every point of the axis through it
    assert np.abs(s[:, :, :3] @ off + s[:, :, 3] - off).max() < 1e-15
    on_axis = off + 0.07 * np.array(axis) / 3.0
    assert np.abs(s[:, :, :3] @ on_axis + s[:, :, 3] - on_axis).max() < 1e-15
    # an unnormalised axis gives the same set
    s2 = metrics.symmetry_transforms({"symmetries_continuous": [{"axis": [10.0, 20.0, -20.0], "offset": offset_mm}]})
    assert np.abs(s - s2).max() < 1e-15


def test_discrete_and_continuous_order():
    flip_x = [1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, -1.0, 6.0, 0, 0, 0, 1.0]      # half turn about x, 6 mm along z
    entry = {"symmetries_discrete": [flip_x], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}
    s = metrics.symmetry_transforms(entry)
    assert s.shape == (2 * N_CONT, 3, 4)
    cont = metrics.symmetry_transforms({"symmetries_continuous": entry["symmetries_continuous"]})
    assert np.abs(s[:N_CONT] - cont).max() == 0.0                              # d = I outer, c inner
    d = np.array(flip_x).reshape(4, 4)
    d[:3, 3] /= 1000.0
    for i in (0, 1, 100, 314):
        c = np.vstack((cont[i], [0, 0, 0, 1]))
        assert np.abs(s[N_CONT + i] - (c @ d)[:3]).max() < 1e-15               # c o d: R_c R_d, R_c t_d + t_c
    assert abs(s[N_CONT][2, 3] - 0.006) < 1e-18                                # millimetres came back as metres


def test_millimetres_become_metres():
    T = np.eye(4)
    T[:3, :3] = np.diag([-1.0, -1.0, 1.0])
    T[:3, 3] = [12.0, -34.0, 56.0]
    s = metrics.symmetry_transforms({"symmetries_discrete": [T.reshape(16).tolist()]})
    assert np.abs(s[1][:, 3] - [0.012, -0.034, 0.056]).max() < 1e-18


def test_two_continuous_axes_compose_in_file_order():
    e = {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}, {"axis": [1, 0, 0], "offset": [0, 0, 0]}]}
    s = metrics.symmetry_transforms(e, max_sym_disc_step=0.5)       # N = 7
    assert s.shape == (49, 3, 4)
    a = metrics.symmetry_transforms({"symmetries_continuous": e["symmetries_continuous"][:1]}, 0.5)
    b = metrics.symmetry_transforms({"symmetries_continuous": e["symmetries_continuous"][1:]}, 0.5)
    assert np.abs(s[3 * 7 + 5][:, :3] - b[5][:, :3] @ a[3][:, :3]).max() < 1e-15


def test_rejects_zero_axis_and_non_orthonormal_block():
    with pytest.raises(ValueError, match="10"):
        metrics.symmetry_transforms({"symmetries_continuous": [{"axis": [0, 0, 0], "offset": [0, 0, 0]}]}, obj_id=10)
    bad = list(HALF_TURN_Z)
    bad[0] = -1.001
    with pytest.raises(ValueError, match="11"):
        metrics.symmetry_transforms({"symmetries_discrete": [bad]}, obj_id=11)
    ok = list(HALF_TURN_Z)
    ok[0] = -1.0 - 1e-8                 # within 1e-6 of orthonormal
    assert len(metrics.symmetry_transforms({"symmetries_discrete": [ok]}, obj_id=11)) == 2


# ------------------------------------------------------------------------------------------------- mssd_err / mspd_err

def test_identity_set_is_the_plain_maximum():
    rng = np.random.default_rng(1)
    model = rng.normal(size=(300, 3)) * [0.05, 0.04, 0.03]
    for _ in range(5):
        g = rand_pose(rng)
        e = perturb(rng, g)
        a, b = model @ g[:3, :3].T + g[:3, 3], model @ e[:3, :3].T + e[:3, 3]
        pa, pb = a @ CAM.T, b @ CAM.T
        want_3d = np.linalg.norm(a - b, axis=1).max()
        want_2d = np.linalg.norm(pa[:, :2] / pa[:, 2:] - pb[:, :2] / pb[:, 2:], axis=1).max()
        assert abs(metrics.mssd_err(g, e, model, IDENTITY) - want_3d) < 1e-15
        assert abs(metrics.mspd_err(g, e, model, CAM, IDENTITY) - want_2d) < 1e-11
        assert metrics.mssd_err(g, e, model, IDENTITY) >= metrics.add_err(g, e, model)
        assert metrics.mspd_err(g, e, model, CAM, IDENTITY) >= metrics.projection_error_2d(g, e, model, CAM)


def test_identical_pose_is_exactly_zero():
    rng = np.random.default_rng(2)
    model = rng.normal(size=(200, 3)) * 0.05
    g = rand_pose(rng)
    syms = metrics.symmetry_transforms({"symmetries_discrete": [HALF_TURN_Z]})
    assert metrics.mssd_err(g, g, model, syms) == 0.0
    assert metrics.mspd_err(g, g, model, CAM, syms) == 0.0


def test_half_turn_needs_the_half_turn():
    rng = np.random.default_rng(3)
    half = rng.normal(size=(400, 3)) * 0.05
    model = np.concatenate([half, half * [-1, -1, 1]])
    g = rand_pose(rng)
    e = g @ np.diag([-1.0, -1.0, 1.0, 1.0])
    with_turn = metrics.symmetry_transforms({"symmetries_discrete": [HALF_TURN_Z]})
    assert metrics.mssd_err(g, e, model, with_turn) <= 1e-12
    assert metrics.mspd_err(g, e, model, CAM, with_turn) <= 1e-9
    assert metrics.mssd_err(g, e, model, IDENTITY) > 1e-2


def circles(rng, n=500, r_max=0.05):
    """Points on circles about z; the largest radius is r_max exactly."""
    r = rng.uniform(0.005, r_max, size=n)
    r[7] = r_max
    a = rng.uniform(0, 2 * np.pi, size=n)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-0.03, 0.03, size=n)], axis=1), r_max


@pytest.mark.parametrize("phi", [0.004, 0.0131, 1.0, 2.5, -0.77, 2 * np.pi / 315 * 40.5])
def test_surface_of_revolution(phi):
    rng = np.random.default_rng(4)
    model, r_max = circles(rng)
    syms = metrics.symmetry_transforms({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})
    g = rand_pose(rng)
    step = 2 * np.pi / N_CONT
    delta = abs(phi - step * np.round(phi / step))
    assert abs(metrics.mssd_err(g, g @ rz44(phi), model, syms) - 2 * r_max * np.sin(delta / 2)) < 1e-12


def test_pose_errors_sym_host_columns():
    rng = np.random.default_rng(5)
    model = rng.normal(size=(100, 3)) * 0.05
    syms = metrics.symmetry_transforms({"symmetries_discrete": [HALF_TURN_Z]})
    gts = np.stack([rand_pose(rng) for _ in range(3)])
    ests = np.stack([perturb(rng, g) for g in gts])
    mssd, mspd = metrics.pose_errors_sym(gts, ests[:, :3], model, CAM, syms)
    for p in range(3):
        assert mssd[p] == metrics.mssd_err(gts[p], ests[p], model, syms)
        assert mspd[p] == metrics.mspd_err(gts[p], ests[p], model, CAM, syms)
    a, b = metrics.pose_errors_sym(gts, ests, model, CAM, syms, want=metrics.WANT_MSSD)
    assert np.array_equal(a, mssd) and np.isnan(b).all()
    a, b = metrics.pose_errors_sym(gts, ests, model, None, syms, want=metrics.WANT_MSSD)
    assert np.array_equal(a, mssd)
    a, b = metrics.pose_errors_sym(gts, ests, model, CAM, syms, want=metrics.WANT_MSPD)
    assert np.isnan(a).all() and np.array_equal(b, mspd)


# ---------------------------------------------------------------------------------------------------- evaluate_results

def hand_made_run(frames=24):
    """Estimates whose errors spread over the ten thresholds: translations of 2.1 .. 71.1 mm along the camera's x axis,
    every third one turned half-way about z, every fifth box off."""
    rng = np.random.default_rng(6)
    half = rng.normal(size=(150, 3)) * 0.03
    model = np.concatenate([half, half * [-1, -1, 1]])
    final_result, gt_frames = [], {}
    for nr in range(frames):
        g = rand_pose(rng)
        e = g.copy()
        e[0, 3] += 0.0021 + 0.003 * nr
        if nr % 3 == 1:
            e = e @ np.diag([-1.0, -1.0, 1.0, 1.0])
        box = [100.0 + nr, 80.0, 80.0, 90.0]
        off = 60.0 if nr % 5 == 4 else 2.0
        gt_frames[nr] = [{"pose": g, "bbox": box}]
        final_result.append({"imgname": "%04d.png" % nr, "cam_R": e[:3, :3], "cam_t": e[:3, 3:4],
                             "result": [{"bbox": [box[0] + off, box[1], box[0] + box[2] + off, box[1] + box[3]]}]})
    return final_result, gt_frames, model


def test_evaluate_results_recalls():
    fr, gtf, model = hand_made_run()
    syms = metrics.symmetry_transforms({"symmetries_discrete": [HALF_TURN_Z]})
    diameter = 100.0
    before = metrics.evaluate_results(fr, gtf, model, CAM, diameter)
    assert set(before) == {"mean_add", "mean_2d_acc", "mean_iou", "mean_add_err_mm", "n"}
    assert set(metrics.evaluate_results(fr, gtf, model, CAM, diameter, symmetries=None)) == set(before)
    m = metrics.evaluate_results(fr, gtf, model, CAM, diameter, symmetries=syms)
    assert set(m) - set(before) == {"ar_mssd", "ar_mspd", "mean_mssd_err_mm", "mean_mspd_err_px"}
    assert {k: m[k] for k in before} == before
    scored = [nr for nr in range(len(fr)) if nr % 5 != 4]           # the others' boxes miss (IoU < 0.5)
    mssd, mspd = [], []
    for nr in scored:
        e = np.eye(4)
        e[:3, :3], e[:3, 3] = fr[nr]["cam_R"], fr[nr]["cam_t"][:, 0]
        mssd.append(metrics.mssd_err(gtf[nr][0]["pose"], e, model, syms) * 1000)
        mspd.append(metrics.mspd_err(gtf[nr][0]["pose"], e, model, CAM, syms))
    mssd, mspd = np.array(mssd), np.array(mspd)
    want_mssd = np.mean([np.mean(mssd < th * diameter) for th in np.arange(1, 11) * 0.05])
    want_mspd = np.mean([np.mean(mspd < th) for th in np.arange(1, 11) * 5.0])
    assert m["ar_mssd"] == pytest.approx(want_mssd, abs=1e-15) and 0.0 < m["ar_mssd"] < 1.0
    assert m["ar_mspd"] == pytest.approx(want_mspd, abs=1e-15) and 0.0 < m["ar_mspd"] < 1.0
    assert m["mean_mssd_err_mm"] == pytest.approx(mssd.mean(), abs=1e-12)
    assert m["mean_mspd_err_px"] == pytest.approx(mspd.mean(), abs=1e-12)
    # the turned estimates count only with the half turn in the set, and a wider image loosens the pixel thresholds
    plain = metrics.evaluate_results(fr, gtf, model, CAM, diameter, symmetries=IDENTITY)
    assert plain["ar_mssd"] < m["ar_mssd"] and plain["ar_mspd"] < m["ar_mspd"]
    wide = metrics.evaluate_results(fr, gtf, model, CAM, diameter, symmetries=syms, image_width=1280)
    want_wide = np.mean([np.mean(mspd < th * 2.0) for th in np.arange(1, 11) * 5.0])
    assert wide["ar_mspd"] == pytest.approx(want_wide, abs=1e-15) and wide["ar_mspd"] > m["ar_mspd"]
    assert wide["ar_mssd"] == m["ar_mssd"]


# ------------------------------------------------------------------------------------------------------ write_sixd_tree

def one_object_tree(path, **kw):
    R = np.eye(3)
    synth.write_sixd_tree(str(path), 1, {0: [(1, R, [0.0, 0.0, 800.0], [10.0, 20.0, 30.0, 40.0])]},
                          {1: np.zeros((3, 3))}, {1: np.zeros((3, 3))}, {1: 100.0}, **kw)


def test_models_info_bytes_without_the_keyword(tmp_path):
    one_object_tree(tmp_path / "a")
    one_object_tree(tmp_path / "b", symmetries=None)
    for d in ("a", "b"):
        with open(tmp_path / d / "models" / "models_info.yml", "rb") as f:
            assert f.read() == b"1:\n  diameter: 100.0\n"


def test_write_then_load_symmetries_round_trips(tmp_path):
    T = np.eye(4)
    T[:3, :3] = np.diag([-1.0, 1.0, -1.0])
    T[:3, 3] = [1.5, 0.0, -2.25]
    fields = {"symmetries_discrete": [HALF_TURN_Z, T],
              "symmetries_continuous": [{"axis": [0.0, 0.0, 1.0], "offset": [1.0, 2.0, 3.0]}]}
    one_object_tree(tmp_path, symmetries={1: fields})
    got = metrics.load_symmetries(str(tmp_path), 1)
    want = metrics.symmetry_transforms({"symmetries_discrete": [HALF_TURN_Z, T.reshape(16).tolist()],
                                        "symmetries_continuous": fields["symmetries_continuous"]})
    assert got.shape == (3 * N_CONT, 3, 4) and np.array_equal(got, want)
    # the rest of the tree still loads, and the diameter is still there
    import yaml
    info = yaml.safe_load(open(os.path.join(str(tmp_path), "models", "models_info.yml")))
    assert info[1]["diameter"] == 100.0 and set(info[1]) == {"diameter", "symmetries_discrete", "symmetries_continuous"}
    assert metrics.load_image_width(str(tmp_path)) == 640


def test_load_symmetries_names_the_object(tmp_path):
    one_object_tree(tmp_path, symmetries={1: {"symmetries_continuous": [{"axis": [0, 0, 0], "offset": [0, 0, 0]}]}})
    with pytest.raises(ValueError, match="object 1"):
        metrics.load_symmetries(str(tmp_path), 1)


def test_bop_metrics_flag():
    assert build_parser().parse_args([]).bop_metrics is False
    assert build_parser().parse_args(["--bop_metrics"]).bop_metrics is True
    ns = build_parser().parse_args(["--bop_metrics", "--symmetric_ids", "10,11", "--device_pnp"])
    assert ns.bop_metrics and ns.symmetric_ids == "10,11"
