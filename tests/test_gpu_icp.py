"""bp_icp_normal_equations and bp_refine_depth (csrc/icp.hip) against their host twins on the scenes of test_icp_host.py:
the normal equations within the rounding of an f64 sum and bit-identical between calls; the refined poses with the same
statuses, step counts and pixel counts; identical bits between two calls, chunk sizes and streams; the guards, the
argument checks, metrics.refine_poses_depth(device=...) and the harness flag.

Image sizes (raster_common.SIZES) and what each opens in icp_accumulate_kernel (ICP_PIX = 2 048 pixels per block):
  48 x 64     every test that names no size.  Two whole slices; W divides the block, so a lane keeps one column and the
              border test falls on the same lanes in every row.
  75 x 113    five slices, 4 x 2 048 + 283; W is an odd prime, so a lane's column changes with every pixel and ``i / W`` is
              a division; ``partial[(p * gridDim.x + blockIdx.x) * 29 + k]`` and icp_sum_slices run over five slices
              (chunks of 1 and 3 poses move a pose's rows).
  129 x 67    five slices, the last of 451 pixels; H > W.
              In the random-pose scenes the object ends before the last rows: at 75 x 113 their last slice adds nothing,
              at 129 x 67 only two slices add anything.  test_normal_equations_parity_in_every_slice fills the frame and
              has accepted pixels in every slice at both sizes: 167 of the 283 at 75 x 113 (the 27 second pixels of a
              lane there lie in the border row, which never counts), up to 340 of the 451 at 129 x 67, among them second
              pixels of a lane.
  16 x 16     with 65 538 poses, two more than a grid has columns: the pose loops of the raster kernels and of
              icp_accumulate_kernel iterate again."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import icp_common as ic  # noqa: E402
import raster_common as rc  # noqa: E402
from icp_common import diverged_scene, equations, guard_cases, refine, singular_scene  # noqa: E402

H, W, K = ic.H, ic.W, ic.K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("c", [0.0, 0.5])
@pytest.mark.parametrize("name", ["torus", "box"])
def test_normal_equations_parity_and_repeat(name, c):
    s = ic.scene(name)
    assert ic.threshold_margin(s["start"], s, c) > 1e-9
    want = equations(s, s["start"], pixel_center=c)
    got = equations(s, s["start"], device="cuda", pixel_center=c)
    ic.assert_equations_close(got, want)
    assert np.array_equal(bits(equations(s, s["start"], device="cuda", pixel_center=c)), bits(got))
    assert np.array_equal(bits(equations(s, s["start"], device="cuda", pixel_center=c, chunk=1)), bits(got))
    assert np.array_equal(bits(equations(s, s["start"], device="cuda", pixel_center=c, chunk=3)), bits(got))


def test_normal_equations_without_image_are_zero():
    s = ic.scene("torus")
    index = np.array([0, -1, 2, 9], np.int32)
    got = equations(dict(s, index=index), s["start"], device="cuda")
    want = equations(dict(s, index=index), s["start"])
    assert np.all(got[[1, 3]] == 0) and np.all(want[[1, 3]] == 0)
    ic.assert_equations_close(got, want)


def assert_refined_like_host(got, want):
    """Same status, iterations_done and N_* for every pose; poses within the tolerance used for numpy-vs-host."""
    assert np.array_equal(got[1][:, [0, 2, 4, 5]], want[1][:, [0, 2, 4, 5]])
    assert np.abs(got[0] - want[0]).max() <= ic.POSE_TOL
    assert np.allclose(got[1][:, [1, 3]], want[1][:, [1, 3]], rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", ["torus", "box"])
def test_refine_parity_repeat_chunks_and_stream(name):
    check_refine_parity_repeat_chunks_and_stream(name, rc.SIZE)


def check_refine_parity_repeat_chunks_and_stream(name, size):
    import torch
    s = ic.scene(name, size=size)
    want = ic.refined_host(name, size)
    first = refine(s, s["start"], device="cuda")
    assert_refined_like_host(first, want)
    for p in range(len(first[0])):
        assert ic.add(first[0][p], s["gt"][p], s["v"]) < 0.5 * ic.add(s["start"][p], s["gt"][p], s["v"])
    for kw in ({}, {"chunk": 1}, {"chunk": 3}):
        again = refine(s, s["start"], device="cuda", **kw)
        assert np.array_equal(bits(again[0]), bits(first[0])) and np.array_equal(bits(again[1]), bits(first[1])), kw
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = refine(s, s["start"], device="cuda")
    torch.cuda.synchronize()
    assert np.array_equal(bits(other[0]), bits(first[0])) and np.array_equal(bits(other[1]), bits(first[1]))


def test_refine_sliding_and_fewer_iterations():
    s = ic.scene("box", sliding=True)
    assert_refined_like_host(refine(s, s["start"], device="cuda"), refine(s, s["start"]))
    s = ic.scene("torus")
    for it in (0, 1):
        got, want = refine(s, s["start"], device="cuda", iterations=it), refine(s, s["start"], iterations=it)
        assert_refined_like_host(got, want)
        assert np.all(got[1][:, 4] == it)
    assert np.array_equal(bits(refine(s, s["start"], device="cuda", iterations=0)[0]), bits(s["start"]))


@pytest.mark.parametrize("case", ["all_zero", "no_image", "index_T", "far"])
def test_guards_return_the_input(case):
    s = ic.scene("torus")
    test, index, status = guard_cases(s)[case]
    got, stats = refine(s, s["start"], test, index, device="cuda")
    assert np.array_equal(bits(got), bits(s["start"]))
    assert np.all(stats[:, 5] == status) and np.all(stats[:, 4] == 0) and np.all(stats[:, [0, 2]] == 0)


def test_start_at_ground_truth_stays():
    s = ic.scene("torus")
    got, stats = refine(s, s["gt"], device="cuda")
    assert_refined_like_host((got, stats), refine(s, s["gt"]))
    assert np.all(stats[:, 3] <= stats[:, 1])
    for p in range(len(got)):
        assert ic.add(got[p], s["gt"][p], s["v"]) < s["depth_scale"]


def test_diverged_singular_and_mixed_statuses():
    s = diverged_scene()
    got, stats = refine(s, s["start"], device="cuda")
    assert_refined_like_host((got, stats), refine(s, s["start"]))
    assert np.array_equal(stats[:, 5], [ic.OK, ic.DIVERGED, ic.TOO_FEW, ic.OK])
    assert np.array_equal(bits(got[1:3]), bits(s["start"][1:3]))
    s = singular_scene()
    got, stats = refine(s, s["start"], device="cuda")
    assert stats[0, 0] >= 32 and stats[0, 4] == 0 and stats[0, 5] in (ic.SINGULAR, ic.DIVERGED)
    assert np.array_equal(bits(got), bits(s["start"]))
    s = ic.scene("box")
    index = np.array([0, -1, 2, 7], np.int32)
    got, stats = refine(s, s["start"], index=index, device="cuda", chunk=2)
    assert np.array_equal(stats[:, 5], [ic.OK, ic.NO_IMAGE, ic.OK, ic.NO_IMAGE])
    assert np.array_equal(bits(got[[1, 3]]), bits(s["start"][[1, 3]]))
    assert np.abs(got[[0, 2]] - ic.refined_host("box")[0][[0, 2]]).max() <= ic.POSE_TOL


# ---------------------------------------------------------------- the other image sizes, many poses

def size_id(size):
    return "%dx%d" % tuple(size)


@pytest.mark.parametrize("c", [0.0, 0.5])
@pytest.mark.parametrize("name", ["torus", "box"])
@pytest.mark.parametrize("size", rc.SIZES[1:], ids=size_id)
def test_normal_equations_parity_and_repeat_at_size(size, name, c):
    """Five slices per pose, the last ragged, on rows that are no multiple of the block (raster_common.SIZES): within
    the rounding of an f64 sum of the host twin, the same bits between calls and between chunks of 1 and 3 poses (the
    stride of ``partial`` between poses), and N exactly the count of the numpy restatement's mask."""
    s = ic.scene(name, size=size)
    assert ic.threshold_margin(s["start"], s, c) > 1e-9
    want = equations(s, s["start"], pixel_center=c)
    got = equations(s, s["start"], device="cuda", pixel_center=c)
    print(size, name, c, "N", got[:, 27], "worst |device - host| / bound", ic.worst_bound_ratio(got, want))
    ic.assert_equations_close(got, want)
    assert np.array_equal(bits(equations(s, s["start"], device="cuda", pixel_center=c)), bits(got))
    assert np.array_equal(bits(equations(s, s["start"], device="cuda", pixel_center=c, chunk=1)), bits(got))
    assert np.array_equal(bits(equations(s, s["start"], device="cuda", pixel_center=c, chunk=3)), bits(got))
    for p, pose in enumerate(s["start"]):
        take = ic.pixel_terms(ic.render(pose, s["v"], s["f"], c, size=size), s["test"][p].astype(np.float64) * s["depth_scale"],
                              pose, s["max_dist"], s["min_cos"], c, size)["take"]
        assert got[p, 27] == take.sum() and take.sum() >= 200


@pytest.mark.parametrize("c", [0.0, 0.5])
@pytest.mark.parametrize("size", rc.SIZES[1:], ids=size_id)
def test_normal_equations_parity_in_every_slice(size, c):
    """The objects of the random-pose scenes end before the last rows, so the last of their five slices adds nothing.
    icp_common.closeup_scene fills the frame: precondition, from the numpy restatement, every slice of 2 048 pixels
    holds accepted pixels, the ragged last one too, and at 129 x 67 also beyond its first 256 (the second pixel of a
    lane; at 75 x 113 those 27 pixels lie in the border row H - 1, which never counts).  Then the usual bars: the host
    twin within the rounding of an f64 sum, N exactly numpy's, the same bits between calls and chunk sizes."""
    s = ic.closeup_scene(size)
    assert ic.threshold_margin(s["start"], s, c) > 1e-9
    per_slice = np.stack([ic.take_per_slice(pose, p, s, c) for p, pose in enumerate(s["start"])])
    assert per_slice.shape == (2, 5) and per_slice.min() > 0, per_slice
    if size == (129, 67):
        assert ic.take_per_slice(s["start"][1], 1, s, c, pixels=256)[33:].sum() > 0     # flat index >= 4 * 2 048 + 256
    want = equations(s, s["start"], pixel_center=c)
    got = equations(s, s["start"], device="cuda", pixel_center=c)
    ic.assert_equations_close(got, want)
    assert np.array_equal(got[:, 27], per_slice.sum(axis=1))
    assert np.array_equal(bits(equations(s, s["start"], device="cuda", pixel_center=c)), bits(got))
    assert np.array_equal(bits(equations(s, s["start"], device="cuda", pixel_center=c, chunk=1)), bits(got))


def test_refine_parity_repeat_chunks_and_stream_at_75x113():
    s = ic.scene("torus", size=(75, 113))
    assert ic.threshold_margin(s["start"], s) > 1e-9
    assert ic.condition_numbers(equations(s, s["start"])).max() < ic.COND_MAX       # what POSE_TOL's derivation assumes
    check_refine_parity_repeat_chunks_and_stream("torus", (75, 113))


def test_guard_returns_the_input_at_75x113():
    """The guard whose pixels are all looked at and all refused: test images one diameter too deep."""
    s = ic.scene("torus", size=(75, 113))
    test, index, status = guard_cases(s)["far"]
    assert test.shape == s["test"].shape and test.max() > 0
    got, stats = refine(s, s["start"], test, index, device="cuda")
    assert np.array_equal(bits(got), bits(s["start"]))
    assert np.all(stats[:, 5] == status) and np.all(stats[:, 4] == 0) and np.all(stats[:, [0, 2]] == 0)


def test_normal_equations_more_poses_than_a_grid_has_columns():
    """65 538 poses on a 16 x 16 image, cycling through 7 (icp_common.many_scene): the pose loops of the raster kernels
    and of icp_accumulate_kernel take a second iteration.  The 7 poses alone are held to the host twin; row p of the
    long call equals row p % 7 of that device result bit for bit."""
    s = ic.many_scene()
    assert ic.threshold_margin(s["start"], s) > 1e-9
    seven = equations(s, s["start"], device="cuda")
    ic.assert_equations_close(seven, equations(s, s["start"]))
    assert seven[:, 27].min() >= 32 and len({r.tobytes() for r in seven}) == len(seven)
    cycle = np.arange(rc.MANY) % len(seven)
    many = equations(dict(s, index=s["index"][cycle]), s["start"][cycle], device="cuda")
    whole = rc.MANY // len(seven) * len(seven)
    assert np.array_equal(bits(many[:whole]).reshape(-1, len(seven), ic.ACC),
                          np.broadcast_to(bits(seven), (whole // len(seven),) + seven.shape))
    assert np.array_equal(bits(many[whole:]), bits(seven[:rc.MANY - whole]))


def test_refine_rejects_bad_arguments():
    import torch
    from betapose_amd import _lib
    s = ic.scene("box")
    L, p = _lib.lib(), _lib.ptr
    P = len(s["start"])
    d_model, d_faces = torch.from_numpy(np.array(s["v"])).cuda(), torch.from_numpy(np.array(s["f"])).cuda()
    d_poses = torch.from_numpy(np.array(s["start"]).reshape(P, 12)).cuda()
    d_test = torch.from_numpy(np.array(s["test"]).view(np.int16)).cuda()
    d_index = torch.from_numpy(np.array(s["index"])).cuda()
    d_out = torch.zeros((P, 12), dtype=torch.float64, device="cuda")
    d_stats = torch.zeros((P, 6), dtype=torch.float64, device="cuda")
    d_acc = torch.zeros((P, 29), dtype=torch.float64, device="cuda")
    Kf = np.ascontiguousarray(K).reshape(9)
    stream = torch.cuda.current_stream().cuda_stream
    good = [p(d_model), len(s["v"]), p(d_faces), len(s["f"]), p(d_poses), P, p(Kf), p(d_test), len(s["test"]), H, W,
            s["depth_scale"], p(d_index), 8, s["max_dist"], 0.25, 32, 0.0, 0.01, 0, p(d_out), p(d_stats), stream]
    assert L.bp_refine_depth(*good) == 0
    assert np.array_equal(d_stats.cpu().numpy()[:, 5], np.zeros(P))
    for i, val in [(0, None), (2, None), (4, None), (6, None), (7, None), (12, None), (20, None), (21, None), (1, 0), (3, 0),
                   (5, 0), (8, 0), (9, 0), (10, -1), (11, 0.0), (13, -1), (14, 0.0), (15, 1.5), (16, -1), (18, 0.0), (19, -1),
                   (20, p(d_poses))]:
        args = list(good)
        args[i] = val
        assert L.bp_refine_depth(*args) < 0, i
        assert len(L.bp_last_error()) > 0
    args = list(good)
    args[9], args[10] = 4097, 4096             # H * W > 2^24 (refused before anything is touched)
    assert L.bp_refine_depth(*args) < 0
    good = [p(d_model), len(s["v"]), p(d_faces), len(s["f"]), p(d_poses), P, p(Kf), p(d_test), len(s["test"]), H, W,
            s["depth_scale"], p(d_index), s["max_dist"], 0.25, 0.0, 0.01, 0, p(d_acc), stream]
    assert L.bp_icp_normal_equations(*good) == 0 and d_acc.cpu().numpy()[:, 27].min() > 0
    for i, val in [(0, None), (2, None), (4, None), (6, None), (7, None), (12, None), (18, None), (1, 0), (3, 0), (5, 0), (8, 0),
                   (9, 0), (10, -1), (11, 0.0), (13, 0.0), (14, -0.1), (16, 0.0), (17, -1)]:
        args = list(good)
        args[i] = val
        assert L.bp_icp_normal_equations(*args) < 0, i


def test_refine_bad_face_index_is_skipped():
    """The device call cannot refuse an index it has not read: the rasteriser skips the triangle, as in bp_render_depth."""
    s = ic.scene("box")
    bad = np.array(s["f"])
    bad[3, 1] = len(s["v"])
    keep = np.ones(len(bad), bool)
    keep[3] = False
    from betapose_amd import _lib
    import torch
    P = len(s["start"])
    L, p = _lib.lib(), _lib.ptr
    d_model, d_faces = torch.from_numpy(np.array(s["v"])).cuda(), torch.from_numpy(bad).cuda()
    d_poses = torch.from_numpy(np.array(s["start"]).reshape(P, 12)).cuda()
    d_test = torch.from_numpy(np.array(s["test"]).view(np.int16)).cuda()
    d_index = torch.from_numpy(np.array(s["index"])).cuda()
    d_acc = torch.zeros((P, 29), dtype=torch.float64, device="cuda")
    assert L.bp_icp_normal_equations(p(d_model), len(s["v"]), p(d_faces), len(bad), p(d_poses), P,
                                     p(np.ascontiguousarray(K).reshape(9)), p(d_test), len(s["test"]), H, W, s["depth_scale"],
                                     p(d_index), s["max_dist"], 0.25, 0.0, 0.01, 0, p(d_acc),
                                     torch.cuda.current_stream().cuda_stream) == 0
    ic.assert_equations_close(d_acc.cpu().numpy(), equations(dict(s, f=bad[keep]), s["start"]))


def test_evaluate_results_refine_depth_on_device():
    from betapose_amd import metrics
    from test_icp_host import harness_inputs
    s, final, gt_frames, depth_frames = harness_inputs()
    m = metrics.evaluate_results(final, gt_frames, s["v"], K, s["d"] * 1000.0, device="cuda", faces=s["f"],
                                 depth_frames=depth_frames, depth_scale=s["depth_scale"],
                                 refine_depth={"max_dist": s["max_dist"], "min_cos": s["min_cos"]})
    assert (m["refined"], m["rejected"], m["unchanged"]) == (len(final), 0, 0)
    ref = ic.refined_host("torus")[0]
    for nr, f in enumerate(final):
        assert np.array_equal(f["pose_rgb"][:3], s["start"][nr])
        assert np.abs(np.hstack([f["cam_R"], f["cam_t"]]) - ref[nr]).max() <= ic.POSE_TOL


def test_harness_refine_depth_flag(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--synthetic", "4", "--outdir", str(tmp_path / "out"),
                        "--refine_depth", "--device_pnp", "--fused"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("Depth refinement for seq")]
    assert len(lines) == 1, r.stdout[-2000:]
    assert "refined" in lines[0] and "rejected" in lines[0] and "mean rms" in lines[0]
    assert "Mean add accuracy for seq" in r.stdout and "Mean vsd recall" not in r.stdout
