"""The depth refinement on the host: bp_icp_normal_equations_host and bp_refine_depth_host against the numpy restatement
of the definition (icp_common.py), the guards, the argument checks and evaluate_results(refine_depth=...).  No GPU."""
import numpy as np
import pytest

import icp_common as ic
from betapose_amd import metrics
from icp_common import diverged_scene, equations, guard_cases, refine, singular_scene

H, W, K = ic.H, ic.W, ic.K


@pytest.mark.parametrize("c", [0.0, 0.5])
@pytest.mark.parametrize("name", ["torus", "box"])
def test_normal_equations_match_the_definition(name, c):
    s = ic.scene(name)
    # precondition: no pixel's decision hangs on the last bits of a threshold
    assert ic.threshold_margin(s["start"], s, c) > 1e-9
    want = ic.normal_equations_np(s["start"], s["v"], s["f"], s["test"], s["index"], s["depth_scale"], s["max_dist"],
                                  s["min_cos"], c)
    assert want[:, 27].min() >= 200           # the scene is not vacuous
    got = equations(s, s["start"], pixel_center=c)
    ic.assert_equations_close(got, want)


def test_normal_equations_thresholds_take_pixels_out():
    s = ic.scene("torus")
    base = equations(s, s["start"])[:, 27]
    tight = dict(s, max_dist=s["max_dist"] / 8)
    steep = dict(s, min_cos=0.8)
    for other in (tight, steep):
        assert ic.threshold_margin(s["start"], other) > 1e-9
        want = ic.normal_equations_np(s["start"], s["v"], s["f"], s["test"], s["index"], s["depth_scale"], other["max_dist"],
                                      other["min_cos"])
        assert np.all(want[:, 27] < base) and want[:, 27].min() > 0
        ic.assert_equations_close(equations(other, s["start"]), want)


@pytest.mark.parametrize("name", ["torus", "box"])
def test_refinement_halves_add(name):
    """Start poses: the ground truth turned by 3 degrees about a random axis and moved by 3 % of the diameter (ADD
    0.033 .. 0.036 diameters).  The numpy definition alone, measured on these scenes: torus ADD 0.0935 / 0.0936 / 0.0944 /
    0.0969 -> 1.1e-5 / 5.9e-6 / 2.6e-5 / 2.2e-5 (diameter 2.8); box 0.0600 / 0.0615 / 0.0594 / 0.0618 -> 5.7e-6 / 3.8e-6 /
    3.3e-6 / 6.6e-6 (diameter 1.73); every pose takes all 8 steps.  The box's ground truths show three faces each
    (icp_common.ground_truth says why; test_box_sliding_poses covers the others)."""
    s = ic.scene(name)
    want, want_stats = ic.refined_np(name)
    for p in range(len(want)):                # the definition itself meets the condition on these perturbations
        assert ic.add(want[p], s["gt"][p], s["v"]) < 0.5 * ic.add(s["start"][p], s["gt"][p], s["v"])
    got, stats = ic.refined_host(name)
    for p in range(len(got)):
        before, after = ic.add(s["start"][p], s["gt"][p], s["v"]), ic.add(got[p], s["gt"][p], s["v"])
        assert after < 0.5 * before, (p, before, after)
    assert np.array_equal(stats[:, [0, 2, 4, 5]], want_stats[:, [0, 2, 4, 5]])
    assert np.all(stats[:, 5] == ic.OK) and np.all(stats[:, 4] == 8)
    assert np.abs(got - want).max() <= ic.POSE_TOL
    assert np.allclose(stats[:, [1, 3]], want_stats[:, [1, 3]], rtol=1e-6, atol=0)
    assert np.all(stats[:, 3] < stats[:, 1])


SIZE = (75, 113)      # five slices of the device's accumulation, the last ragged (raster_common.SIZES); here: N three times as large


@pytest.mark.parametrize("c", [0.0, 0.5])
def test_normal_equations_match_the_definition_at_75x113(c):
    s = ic.scene("torus", size=SIZE)
    assert s["test"].shape[1:] == SIZE
    assert ic.threshold_margin(s["start"], s, c) > 1e-9
    want = ic.normal_equations_np(s["start"], s["v"], s["f"], s["test"], s["index"], s["depth_scale"], s["max_dist"],
                                  s["min_cos"], c, SIZE)
    assert want[:, 27].min() >= 200
    cond = ic.condition_numbers(want)
    assert cond.max() < ic.COND_MAX, cond           # what POSE_TOL's derivation assumes
    got = equations(s, s["start"], pixel_center=c)
    print("N", want[:, 27], "cond(A)", cond, "worst |host - numpy| / bound", ic.worst_bound_ratio(got, want))
    ic.assert_equations_close(got, want)             # (entry 27, N, exactly)


@pytest.mark.parametrize("size", [(75, 113), (129, 67)], ids=["75x113", "129x67"])
def test_normal_equations_match_the_definition_on_a_filled_frame(size):
    """icp_common.closeup_scene: accepted pixels in every row but the border's (the scene the device test uses to feed
    every slice of its accumulation), about 8 000 terms per sum."""
    s = ic.closeup_scene(size)
    assert ic.threshold_margin(s["start"], s) > 1e-9
    assert np.stack([ic.take_per_slice(pose, p, s) for p, pose in enumerate(s["start"])]).min() > 0
    want = ic.normal_equations_np(s["start"], s["v"], s["f"], s["test"], s["index"], s["depth_scale"], s["max_dist"],
                                  s["min_cos"], 0.0, size)
    assert want[:, 27].min() >= 7000
    ic.assert_equations_close(equations(s, s["start"]), want)


def test_refinement_at_75x113():
    """test_refinement_halves_add for the torus on the larger image: the same assertions and bars, after their
    preconditions (every start pose's threshold margin and cond(A) below COND_MAX)."""
    s = ic.scene("torus", size=SIZE)
    assert ic.threshold_margin(s["start"], s) > 1e-9
    assert ic.condition_numbers(equations(s, s["start"])).max() < ic.COND_MAX
    want, want_stats = ic.refined_np("torus", SIZE)
    got, stats = ic.refined_host("torus", SIZE)
    for p in range(len(got)):
        before, after = ic.add(s["start"][p], s["gt"][p], s["v"]), ic.add(got[p], s["gt"][p], s["v"])
        assert after < 0.5 * before, (p, before, after)
    assert np.array_equal(stats[:, [0, 2, 4, 5]], want_stats[:, [0, 2, 4, 5]])
    assert np.all(stats[:, 5] == ic.OK) and np.all(stats[:, 4] == 8)
    print("N_first", stats[:, 0], "worst |host - numpy| of a pose entry", np.abs(got - want).max())
    assert np.abs(got - want).max() <= ic.POSE_TOL
    assert np.allclose(stats[:, [1, 3]], want_stats[:, [1, 3]], rtol=1e-6, atol=0)
    assert np.all(stats[:, 3] < stats[:, 1])


def test_box_sliding_poses():
    """Two cube poses that show fewer than three faces inside min_cos: the residual still falls (or the pose is given
    back), and the host twin still follows the definition; nothing is claimed about the distance to the ground truth."""
    s = ic.scene("box", sliding=True)
    want, want_stats = ic.refine_np(s["start"], s["v"], s["f"], s["test"], s["index"], s["depth_scale"], max_dist=s["max_dist"],
                                    min_cos=s["min_cos"])
    got, stats = refine(s, s["start"])
    assert np.array_equal(stats[:, [0, 2, 4, 5]], want_stats[:, [0, 2, 4, 5]])
    assert np.all(stats[:, 3] <= stats[:, 1])
    assert np.abs(got - want).max() <= 1e-7       # cond(A) reaches 1.5e3 at the start and grows as the pose slides


@pytest.mark.parametrize("name", ["torus", "box"])
def test_start_at_ground_truth_stays(name):
    s = ic.scene(name)
    got, stats = refine(s, s["gt"])
    assert np.all(stats[:, 3] <= stats[:, 1])
    assert np.all(np.isin(stats[:, 5], [ic.OK, ic.REJECTED]))
    for p in range(len(got)):
        assert ic.add(got[p], s["gt"][p], s["v"]) < s["depth_scale"]       # less than one depth quantum


def test_iterations_zero_only_measures():
    s = ic.scene("torus")
    got, stats = refine(s, s["start"], iterations=0)
    assert np.array_equal(got, s["start"])
    assert np.all(stats[:, 5] == ic.OK) and np.all(stats[:, 4] == 0)
    assert np.array_equal(stats[:, 0], stats[:, 2]) and np.array_equal(stats[:, 1], stats[:, 3])
    assert np.array_equal(stats[:, 0], equations(s, s["start"])[:, 27])


def test_fewer_iterations_end_further_away():
    s = ic.scene("torus")
    one = refine(s, s["start"], iterations=1)
    want = ic.refine_np(s["start"], s["v"], s["f"], s["test"], s["index"], s["depth_scale"], iterations=1,
                        max_dist=s["max_dist"], min_cos=s["min_cos"])
    assert np.abs(one[0] - want[0]).max() <= ic.POSE_TOL and np.all(one[1][:, 4] == 1)
    full = ic.refined_host("torus")[0]
    for p in range(len(full)):
        assert ic.add(full[p], s["gt"][p], s["v"]) < ic.add(one[0][p], s["gt"][p], s["v"])


# ---------------------------------------------------------------- guards

@pytest.mark.parametrize("case", ["all_zero", "no_image", "index_T", "far"])
def test_guards_return_the_input(case):
    s = ic.scene("torus")
    test, index, status = guard_cases(s)[case]
    if case == "far":
        assert test.max() > 0
    got, stats = refine(s, s["start"], test, index)
    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(s["start"]).view(np.uint64))
    assert np.all(stats[:, 5] == status) and np.all(stats[:, 4] == 0) and np.all(stats[:, [0, 2]] == 0)


def test_min_pixels_is_a_guard():
    s = ic.scene("torus")
    n = equations(s, s["start"])[:, 27]
    got, stats = refine(s, s["start"], min_pixels=int(n[1]) + 1)
    want = np.where(n < n[1] + 1, ic.TOO_FEW, ic.OK)
    assert np.array_equal(stats[:, 5], want) and (want == ic.OK).any()
    assert np.array_equal(got[want == ic.TOO_FEW], s["start"][want == ic.TOO_FEW])


def test_diverged_keeps_the_pose_before_the_step():
    s = diverged_scene()
    got, stats = refine(s, s["start"])
    want, want_stats = ic.refine_np(s["start"], s["v"], s["f"], s["test"], s["index"], s["depth_scale"], max_dist=s["max_dist"],
                                    min_cos=s["min_cos"])
    assert np.array_equal(stats[:, [0, 2, 4, 5]], want_stats[:, [0, 2, 4, 5]])
    assert np.array_equal(stats[:, 5], [ic.OK, ic.DIVERGED, ic.TOO_FEW, ic.OK])
    assert stats[1, 0] >= 32 and stats[1, 4] == 0
    assert np.array_equal(got[1:3], s["start"][1:3])


def test_singular_system_is_refused():
    s = singular_scene()
    got, stats = refine(s, s["start"])
    assert stats[0, 0] >= 32 and stats[0, 4] == 0 and stats[0, 5] in (ic.SINGULAR, ic.DIVERGED)
    assert np.array_equal(got, s["start"])


def test_mixed_images_and_statuses():
    """Poses of one call are independent: a pose without an image between two with one."""
    s = ic.scene("box")
    index = np.array([0, -1, 2, 7], np.int32)
    got, stats = refine(s, s["start"], index=index)
    ref = ic.refined_host("box")
    assert np.array_equal(stats[:, 5], [ic.OK, ic.NO_IMAGE, ic.OK, ic.NO_IMAGE])
    assert np.array_equal(got[[0, 2]], ref[0][[0, 2]]) and np.array_equal(got[[1, 3]], s["start"][[1, 3]])


# ---------------------------------------------------------------- arguments

def test_refine_rejects_bad_arguments():
    from betapose_amd import _lib
    s = ic.scene("box")
    v, f = np.array(s["v"]), np.array(s["f"])
    bad = f.copy()
    bad[3, 1] = len(v)
    with pytest.raises(ValueError):
        metrics.refine_poses_depth(s["start"], v, bad, K, s["test"], s["index"])
    with pytest.raises(ValueError):
        metrics.refine_poses_depth(s["start"], v, f, K, s["test"].astype(np.int32), s["index"])
    with pytest.raises(ValueError):
        metrics.refine_poses_depth(s["start"], v, f, K, s["test"], s["index"][:2])
    L = _lib.lib()
    p = _lib.ptr
    P = len(s["start"])
    poses, test, index = np.array(s["start"]), np.array(s["test"]), np.array(s["index"])
    Kf = np.ascontiguousarray(K).reshape(9)
    out, stats, acc = np.zeros((P, 12)), np.zeros((P, 6)), np.zeros((P, 29))
    good = [p(poses), P, p(v), len(v), p(f), len(f), p(Kf), p(test), len(test), H, W, s["depth_scale"], p(index), 8,
            s["max_dist"], 0.25, 32, 0.0, 0.01, p(out), p(stats)]
    assert L.bp_refine_depth_host(*good) == 0
    for i, val in [(0, None), (2, None), (4, None), (6, None), (7, None), (12, None), (19, None), (20, None), (1, 0), (3, 0),
                   (5, 0), (8, 0), (9, 0), (10, -1), (11, 0.0), (13, -1), (14, 0.0), (15, 1.5), (16, -1), (18, 0.0)]:
        args = list(good)
        args[i] = val
        assert L.bp_refine_depth_host(*args) < 0, i
        assert len(L.bp_last_error()) > 0
    args = list(good)
    args[9], args[10] = 4097, 4096             # H * W > 2^24 (refused before anything is touched)
    assert L.bp_refine_depth_host(*args) < 0
    args = list(good)
    args[4] = p(bad)
    assert L.bp_refine_depth_host(*args) < 0 and b"face index" in L.bp_last_error()
    good = [p(poses), P, p(v), len(v), p(f), len(f), p(Kf), p(test), len(test), H, W, s["depth_scale"], p(index),
            s["max_dist"], 0.25, 0.0, 0.01, p(acc)]
    assert L.bp_icp_normal_equations_host(*good) == 0 and acc[:, 27].min() > 0
    for i, val in [(0, None), (2, None), (4, None), (6, None), (7, None), (12, None), (17, None), (1, 0), (3, 0), (5, 0), (8, 0),
                   (9, 0), (10, -1), (11, 0.0), (13, 0.0), (14, -0.1), (16, 0.0)]:
        args = list(good)
        args[i] = val
        assert L.bp_icp_normal_equations_host(*args) < 0, i
    args = list(good)
    args[4] = p(bad)
    assert L.bp_icp_normal_equations_host(*args) < 0 and b"face index" in L.bp_last_error()


# ---------------------------------------------------------------- harness

def harness_inputs(name="torus"):
    """The scene as evaluate_results sees it: frame nr = pose nr, estimates = the start poses, depth in scene units."""
    s = ic.scene(name)
    final, gt_frames, depth_frames = [], {}, {}
    for nr in range(len(s["gt"])):
        gt = np.vstack([s["gt"][nr], [0, 0, 0, 1]])
        gt_frames[nr] = [{"pose": gt, "bbox": [10, 5, 40, 35]}]
        depth_frames[nr] = s["test"][nr]
        final.append({"imgname": "%04d.png" % nr, "result": [{"bbox": np.array([10.0, 5.0, 50.0, 40.0])}],
                      "cam_R": s["start"][nr][:, :3].copy(), "cam_t": s["start"][nr][:, 3].reshape(3, 1).copy()})
    return s, final, gt_frames, depth_frames


def test_evaluate_results_refine_depth():
    s, final, gt_frames, depth_frames = harness_inputs()
    kw = dict(faces=s["f"], depth_frames=depth_frames, depth_scale=s["depth_scale"])
    base = metrics.evaluate_results(final, gt_frames, s["v"], K, s["d"] * 1000.0, **kw)
    same = metrics.evaluate_results(final, gt_frames, s["v"], K, s["d"] * 1000.0, refine_depth=None, **kw)
    assert set(same) == set(base) and all(same[k] == base[k] for k in base)
    assert all("pose_rgb" not in f for f in final)
    with pytest.raises(ValueError):
        metrics.evaluate_results(final, gt_frames, s["v"], K, s["d"] * 1000.0, refine_depth={})
    m = metrics.evaluate_results(final, gt_frames, s["v"], K, s["d"] * 1000.0,
                                 refine_depth={"max_dist": s["max_dist"], "min_cos": s["min_cos"]}, **kw)
    assert set(m) == set(base) | {"refined", "rejected", "unchanged", "mean_rms_first", "mean_rms_last"}
    assert m["refined"] + m["rejected"] + m["unchanged"] == len(final) == m["refined"]
    assert m["mean_rms_last"] < m["mean_rms_first"] and m["mean_add_err_mm"] < 0.01 * base["mean_add_err_mm"]
    assert m["mean_vsd_err"] <= base["mean_vsd_err"]
    ref = ic.refined_host("torus")[0]
    for nr, f in enumerate(final):
        assert np.array_equal(f["pose_rgb"][:3], s["start"][nr])
        assert np.array_equal(f["cam_R"], ref[nr][:, :3]) and np.array_equal(f["cam_t"][:, 0], ref[nr][:, 3])


def test_evaluate_results_refine_depth_counts_rejections():
    s, final, gt_frames, depth_frames = harness_inputs()
    depth_frames[1] = np.zeros_like(depth_frames[1])          # no depth at all: TOO_FEW, nothing moves
    m = metrics.evaluate_results(final, gt_frames, s["v"], K, s["d"] * 1000.0, faces=s["f"], depth_frames=depth_frames,
                                 depth_scale=s["depth_scale"], refine_depth={"max_dist": s["max_dist"]})
    assert (m["refined"], m["rejected"], m["unchanged"]) == (3, 0, 1)
    assert np.array_equal(final[1]["cam_R"], s["start"][1][:, :3])
