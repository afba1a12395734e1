"""The host side of pose verification by gradient agreement (csrc/verify_host.cpp through bp_image_gradients_host and
bp_gradient_scores_host; metrics.image_gradients, gradient_scores, verify_poses; renderer.verify_6D_poses,
verify_results; the --verify flag): the gradients against a numpy restatement, the scores against a float64 one, the
frame index, chunking, discrimination, the reference's call shape and the harness flag.  No GPU."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import raster_common as rc
import verify_common as vc
from betapose_amd import _lib, metrics, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. gradients against the numpy restatement
@pytest.mark.parametrize("min_sq", [vc.SCENE_MIN_SQ, vc.RENDER_MIN_SQ])
@pytest.mark.parametrize("red", [0, 2])
@pytest.mark.parametrize("size", vc.SIZES)
def test_gradients_equal_the_numpy_restatement(size, red, min_sq):
    """gx, gy and the mask are recovered from the outputs and must be exact: a kept pixel has ``nx mag = gx (1 + e)``
    with |e| a few 2^-24, so |gx e| <= 12240 * 2^-22 < 0.003 and rounding to the nearest integer gives gx back.
    The unit vectors are checked to 2 ulp of float32 against the definition's own float32 steps restated in numpy
    (sqrt of the f32 m2, plus f32 0.001, f32 quotient: all correctly rounded there too), so the difference is expected
    to be 0 and 2 ulp leaves room for a library whose square root is off by one.  Against the EXACT quotient the
    definition itself is farther off than that in rare pixels: the two roundings of the magnitude are up to 1 ulp of it,
    which is up to 2 ulp of a quotient just under a power of two, plus the quotient's own half -- 2.5 ulp at the worst;
    measured over these images 2.14 ulp (one pixel of (70, 130), gx = -27, gy = -129), printed below and bounded by 2.5."""
    names, stack = vc.images(size)
    grads, mags = metrics.image_gradients(stack, red, min_sq)
    gx, gy, kept, unit = vc.gradients_ref(size, red, min_sq)
    assert grads.shape == stack.shape[:3] + (2,) and grads.dtype == np.float32 and mags.dtype == np.float32
    assert np.array_equal(mags > 0, kept)
    assert not grads[~kept].any() and not mags[~kept].any()
    assert np.array_equal(np.rint(grads[..., 0].astype(np.float64) * mags)[kept], gx[kept])
    assert np.array_equal(np.rint(grads[..., 1].astype(np.float64) * mags)[kept], gy[kept])
    want = vc.units_f32_ref(gx, gy, kept)
    ulps = np.abs(grads.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    exact = np.abs(grads.astype(np.float64) - unit) / np.spacing(np.abs(unit).astype(np.float32)).astype(np.float64)
    print("size %s red %d min_sq %d: %.3f ulp from the f32 restatement, %.3f ulp from the exact quotient" % (
        size, red, min_sq, ulps.max(), exact.max()))
    assert ulps.max() <= 2.0
    assert exact.max() <= 2.5
    assert not kept[names.index("constant")].any()
    if min_sq == vc.SCENE_MIN_SQ and size[0] * size[1] > 100:
        low = names.index("low")
        m2 = gx[low] ** 2 + gy[low] ** 2
        assert ((m2 >= 16) & (m2 < 25)).any() and ((m2 >= 25) & (m2 < 37)).any()      # both sides of the integer mask
    for n in ("line_top", "line_bottom", "line_left", "line_right"):
        assert kept[names.index(n)].any() or min_sq == vc.RENDER_MIN_SQ


def test_gradient_argument_errors():
    img = np.zeros((1, 5, 5, 3), np.uint8)
    for bad in (np.zeros((1, 2, 5, 3), np.uint8), np.zeros((1, 5, 2, 3), np.uint8), np.zeros((1, 5, 5, 3), np.float32),
                np.zeros((5, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            metrics.image_gradients(bad)
    with pytest.raises(ValueError):
        metrics.image_gradients(img, red_channel=1)
    L = _lib.lib()
    g = np.zeros((1, 2, 5, 2), np.float32)
    assert L.bp_image_gradients_host(_lib.ptr(img), 1, 2, 5, 0, 25, _lib.ptr(g), None) != 0        # H < 3 refused
    assert L.bp_image_gradients_host(_lib.ptr(img), 1, 5, 5, 1, 25, _lib.ptr(g), None) != 0
    assert L.bp_image_gradients_host(_lib.ptr(img), 1, 5, 5, 0, 25, _lib.ptr(np.zeros((1, 5, 5, 2), np.float32)), None) == 0


# ---------------------------------------------------------------- 2. scores against the float64 restatement
@pytest.mark.parametrize("render_min_sq", [vc.SCENE_MIN_SQ, vc.RENDER_MIN_SQ])
@pytest.mark.parametrize("red", [0, 2])
@pytest.mark.parametrize("size", vc.SIZES)
def test_scores_equal_the_float64_restatement(size, red, render_min_sq):
    """|score - ref| <= 1e-6, derived: a term is at most 1 and comes from two unit vectors of about 1.5 ulp each, two
    products and a sum, each rounded to f32 -- a handful of roundings of 2^-24 = 6e-8, about 3e-7 in all -- and its
    quantisation to a multiple of 2^-24 adds at most 2^-25 = 3e-8.  The score is the mean of the terms (over count + 1),
    so it is off by no more than a term is; the f64 sum and quotient add nothing visible."""
    renders, frames, index = vc.score_case(size)
    scores, sums, counts = metrics.gradient_scores(renders, frames, index, red, render_min_sq)
    want, want_counts = vc.scores_ref(size, red, render_min_sq)
    assert scores.dtype == np.float64 and sums.dtype == np.uint64 and counts.dtype == np.int32
    assert np.array_equal(counts, want_counts)
    print("size %s red %d min_sq %d: max |score - ref| %.3g, counts %s" % (size, red, render_min_sq, np.abs(scores - want).max(),
                                                                          counts.tolist()))
    assert np.abs(scores - want).max() <= 1e-6
    assert np.array_equal(scores, sums.astype(np.float64) / 2.0 ** 24 / (counts + 1))
    # the gradients handed over instead of the frames: the same bytes
    grads = metrics.image_gradients(frames, red)[0]
    again = metrics.gradient_scores(renders, grads, index, red, render_min_sq)
    assert all(np.array_equal(vc.bits(a), vc.bits(b)) for a, b in zip(again, (scores, sums, counts)))


@pytest.mark.parametrize("size", vc.SIZES)
def test_score_identities(size):
    """A render equal to its frame: every kept pixel's term is |n . n| = 1 up to roundings, so the score is at least
    (1 - 1e-3) count / (count + 1).  A constant render keeps nothing: score 0 and count 0."""
    _, stack = vc.images(size)
    index = np.arange(len(stack), dtype=np.int32)
    scores, sums, counts = metrics.gradient_scores(stack, stack, index, 0, vc.SCENE_MIN_SQ)
    assert (scores >= (1 - 1e-3) * counts / (counts + 1)).all() and (scores <= 1.0 + 1e-6).all()
    assert counts[1] > 0 and scores[0] == 0.0 and counts[0] == 0 and sums[0] == 0


# ---------------------------------------------------------------- 3. frame index, empty input
def test_frame_index_out_of_range_rows():
    renders, frames, index = vc.score_case((37, 53))
    good = metrics.gradient_scores(renders, frames, index, 0, vc.SCENE_MIN_SQ)
    bad = index.copy()
    bad[2], bad[5] = -1, len(frames)
    scores, sums, counts = metrics.gradient_scores(renders, frames, bad, 0, vc.SCENE_MIN_SQ)
    for p in range(len(index)):
        if p in (2, 5):
            assert np.isnan(scores[p]) and sums[p] == 0 and counts[p] == -1
        else:
            assert vc.bits(scores)[p] == vc.bits(good[0])[p] and sums[p] == good[1][p] and counts[p] == good[2][p]
    # several poses of one frame: each row is what the pose gets alone
    for p in (0, 3, 6):
        alone = metrics.gradient_scores(renders[p:p + 1], frames, index[p:p + 1], 0, vc.SCENE_MIN_SQ)
        assert vc.bits(alone[0])[0] == vc.bits(good[0])[p] and alone[1][0] == good[1][p] and alone[2][0] == good[2][p]


def test_empty_input():
    frames = vc.images((5, 7))[1][:2]
    scores, sums, counts = metrics.gradient_scores(np.zeros((0, 5, 7, 3), np.uint8), frames, [])
    assert scores.shape == sums.shape == counts.shape == (0,)
    assert _lib.lib().bp_gradient_scores_host(None, None, None, 0, 2, 5, 7, 0, 25, None, None, None) == 0
    v, f, colors = vc.colored_mesh()
    out = metrics.verify_poses(np.zeros((0, 3, 4)), v, f, colors, rc.camera((5, 7)), frames, [])
    assert [len(a) for a in out] == [0, 0, 0, 0]


# ---------------------------------------------------------------- 4. verify_poses: chunking, textures, two frames
@pytest.fixture(scope="module")
def two_frame_scene():
    size = (48, 64)
    pool0, frame0 = vc.disc_scene(0, size)
    pool1, frame1 = vc.disc_scene(1, size)
    poses = np.concatenate([pool0[:4], pool1[:4]])[[0, 4, 1, 5, 2, 6, 3, 7]]          # interleaved frame indices
    index = np.array([0, 1, 0, 1, 0, 1, 0, 1], np.int32)
    return size, poses, np.concatenate([frame0, frame1]), index


def test_verify_poses_does_not_depend_on_chunk(two_frame_scene):
    size, poses, frames, index = two_frame_scene
    v, f, colors = vc.colored_mesh()
    K = rc.camera(size)
    whole = metrics.verify_poses(poses, v, f, colors, K, frames, index, chunk=len(poses))
    assert whole[2].min() > 0
    for chunk in (0, 1, 3):
        part = metrics.verify_poses(poses, v, f, colors, K, frames, index, chunk=chunk)
        assert all(np.array_equal(vc.bits(a), vc.bits(b)) for a, b in zip(part, whole))
    # the renders scored directly: the same rows
    color = metrics.render_color(poses, v, f, colors, K, size)[0]
    direct = metrics.gradient_scores(color, frames, index)
    assert all(np.array_equal(vc.bits(a), vc.bits(b)) for a, b in zip(direct, whole[:3]))


def test_verify_chunk_rule():
    assert metrics.verify_chunk(480, 640, 1000) == (256 << 20) // (480 * 640 * 7) == 124
    assert metrics.verify_chunk(480, 640, 5) == 5 and metrics.verify_chunk(480, 640, 5, 2) == 2
    assert metrics.verify_chunk(4096, 4096, 9) == 2 and metrics.verify_chunk(4096, 4096 * 4, 9) == 1


# ---------------------------------------------------------------- 5. discrimination
@pytest.mark.parametrize("seed", vc.DISC_SEEDS)
@pytest.mark.parametrize("size", vc.DISC_SIZES)
def test_true_pose_wins(size, seed):
    """The true pose against rotations of 10, 20, 45 and 90 degrees about seeded axes and translations of 10 % and 25 %
    of the diameter along seeded directions: it must score highest in every case (a condition, not a tolerance).  On
    the host twin the true pose scores 0.833 .. 0.868 (its silhouette pixels see the background's gradients on their
    outer side) and the best perturbed pose 0.786 .. 0.832; the smallest winning margin of the 8 cases is 0.029
    (size (70, 130), seed 2: 0.8412 against 0.8120)."""
    pool, frame = vc.disc_scene(seed, size)
    v, f, colors = vc.colored_mesh()
    scores, _, counts, _ = metrics.verify_poses(pool, v, f, colors, rc.camera(size), frame, np.zeros(len(pool), np.int32))
    print("size %s seed %d: true %.4f, best other %.4f, counts %s" % (size, seed, scores[0], scores[1:].max(), counts.tolist()))
    assert counts.min() > 0
    assert int(np.argmax(scores)) == 0 and scores[0] > scores[1:].max()


# ---------------------------------------------------------------- 6. verify_6D_poses
class _Model:
    def __init__(self):
        self.vertices, self.indices, c = vc.colored_mesh()
        self.colors = c.astype(np.float64) / 255.0


def _pose44(p):
    return np.vstack([p, [0, 0, 0, 1.0]])


def test_verify_6d_poses_reference_shape():
    """The reference's arguments and return value: two detections with three poses each; the best pose comes back
    after det[:6], a tie goes to the first pose (np.argmax)."""
    size = (48, 64)
    pool, frame = vc.disc_scene(2, size)
    model_map = {"03": _Model()}
    true, off1, off2 = _pose44(pool[0]), _pose44(pool[3]), _pose44(pool[6])
    dets = [[2, 0.9, 1.0, 2.0, 30.0, 40.0, off1, true, off2], [2, 0.8, 0.0, 0.0, 9.0, 9.0, off2, off2.copy(), off1]]
    before = copy.deepcopy(dets)
    # the frame is RGB here and the reference reads BGR: hand both over flipped, as a caller with cv2 frames would
    m = model_map["03"]
    m.colors = m.colors[:, ::-1]
    out = renderer.verify_6D_poses(dets, model_map, rc.camera(size), np.ascontiguousarray(frame[0][:, :, ::-1]))
    assert len(out) == 2 and all(len(d) == 7 for d in out)
    assert out[0][:6] == before[0][:6] and out[0][6] is dets[0][7]
    # detection 1: poses 0 and 1 tie (equal matrices), and either beats or loses to pose 2 -- the winner is never pose 1
    assert out[1][6] is dets[1][6] or out[1][6] is dets[1][8]
    scores = metrics.verify_poses(np.stack([off2[:3], off2[:3], off1[:3]]), m.vertices, m.indices, metrics.colors_u8(m.colors),
                                  rc.camera(size), np.ascontiguousarray(frame[:, :, :, ::-1]), [0, 0, 0], pixel_center=0.5,
                                  red_channel=2)[0]
    assert scores[0] == scores[1] and out[1][6] is dets[1][6 + int(np.argmax(scores))]
    # floats in [0, 1] are the same image
    outf = renderer.verify_6D_poses(dets, model_map, rc.camera(size), frame[0][:, :, ::-1].astype(np.float32) / 255.0)
    assert all(a[6] is b[6] for a, b in zip(out, outf))
    from betapose_amd.compat.utils import utils as compat_utils
    assert compat_utils.verify_6D_poses is renderer.verify_6D_poses


# ---------------------------------------------------------------- 7. verify_results and --verify
def _instance(pose, status=0):
    if pose is None:
        return {"cam_R": [], "cam_t": [], "status": status, "points": 0, "pick": 0, "bbox": np.zeros(4)}
    return {"cam_R": pose[:, :3].copy(), "cam_t": pose[:, 3:4].copy(), "status": status, "points": 10, "pick": 0,
            "bbox": np.zeros(4)}


def test_verify_results(tmp_path):
    from PIL import Image
    size = (48, 64)
    model = _Model()
    frames = []
    for k in range(3):
        pool, frame = vc.disc_scene(k, size)
        Image.fromarray(frame[0]).save(str(tmp_path / ("%04d.png" % k)))
        frames.append(pool)

    def frame_dict(k, inst):
        first = inst[0]
        return {"imgname": "%04d.png" % k, "result": [{}] * len(inst), "cam_R": first["cam_R"], "cam_t": first["cam_t"],
                "boxes": np.zeros((1, 4)), "instances": inst}
    final = [frame_dict(0, [_instance(frames[0][2]), _instance(frames[0][0]), _instance(frames[0][5])]),     # true pose second
             frame_dict(1, [_instance(frames[1][0]), _instance(None, -1), _instance(frames[1][4])]),        # true pose first
             frame_dict(2, [_instance(frames[2][1]), _instance(None, -1)]),                                 # one solved
             {"imgname": "0002.png", "result": [{}], "cam_R": frames[2][0][:, :3], "cam_t": frames[2][0][:, 3:4],
              "boxes": np.zeros((1, 4))}]                                                                   # no instances
    before = copy.deepcopy(final)
    scored, changed = renderer.verify_results(final, model, str(tmp_path), rc.camera(size), batch=2)
    assert (scored, changed) == (2, 1)
    f0, f1 = final[0], final[1]
    assert np.array_equal(f0["cam_R"], frames[0][0][:, :3]) and np.array_equal(np.reshape(f0["cam_t"], 3), frames[0][0][:, 3])
    assert np.array_equal(f0["pose_unverified"]["cam_R"], before[0]["cam_R"])
    assert np.array_equal(f1["cam_R"], before[1]["cam_R"]) and np.array_equal(f1["pose_unverified"]["cam_t"], before[1]["cam_t"])
    sc0 = [s["verify_score"] for s in f0["instances"]]
    assert int(np.argmax(sc0)) == 1 and "verify_score" not in f1["instances"][1] and "verify_score" in f1["instances"][2]
    # the scores are verify_poses' own
    want = metrics.verify_poses(np.stack([frames[0][2], frames[0][0], frames[0][5]]), model.vertices, model.indices,
                                metrics.colors_u8(model.colors), rc.camera(size), vc.disc_scene(0, size)[1], [0, 0, 0])[0]
    assert sc0 == want.tolist()
    # fewer than two solved instances, or none: untouched
    for k in (2, 3):
        assert final[k].keys() == before[k].keys()
        assert np.array_equal(final[k]["cam_R"], before[k]["cam_R"]) and np.array_equal(final[k]["cam_t"], before[k]["cam_t"])
        assert all("verify_score" not in s for s in final[k].get("instances", []))
    # the JSON carries the scores of the scored instances only
    from betapose_amd.pPose_nms import results_to_json_list
    for fr in final:
        fr["result"] = [{"keypoints": np.zeros((2, 2)), "kp_score": np.zeros((2, 1)), "proposal_score": np.zeros(1)}] * len(fr["result"])
    js = results_to_json_list(final)
    assert [("verify_score" in r) for r in js] == [True, True, True, True, False, True, False, False, False]


def test_verify_flag_needs_candidates_and_all_instances(tmp_path):
    for script in ("evaluate.py", "occlusion_evaluate.py"):
        for extra in ([], ["--candidates", "3"]):
            r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--synthetic", "2", "--outdir", str(tmp_path),
                                "--verify"] + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
            assert r.returncode != 0 and "--verify" in r.stderr and "--candidates" in r.stderr and "--all_instances" in r.stderr, r.stderr
