"""Pose verification by gradient agreement on the GPU (csrc/verify.hip through bp_image_gradients and
bp_gradient_scores; metrics.verify_poses; the --verify flag): every output equals the host twin's byte for byte -- on
every image and size of verify_common.py, on a stream of the caller's, from call to call into dirty buffers, through
the renderer (vertex colours and textures, chunked, two frames) and through the harness."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_common as rc  # noqa: E402
import verify_common as vc  # noqa: E402
from betapose_amd import _lib, metrics  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return all(np.array_equal(vc.bits(x), vc.bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("min_sq", [vc.SCENE_MIN_SQ, vc.RENDER_MIN_SQ])
@pytest.mark.parametrize("red", [0, 2])
@pytest.mark.parametrize("size", vc.SIZES)
def test_image_gradients_equal_host(size, red, min_sq):
    _, stack = vc.images(size)
    assert same(metrics.image_gradients(stack, red, min_sq, "cuda"), metrics.image_gradients(stack, red, min_sq))


@pytest.mark.parametrize("render_min_sq", [vc.SCENE_MIN_SQ, vc.RENDER_MIN_SQ])
@pytest.mark.parametrize("red", [0, 2])
@pytest.mark.parametrize("size", vc.SIZES)
def test_gradient_scores_equal_host(size, red, render_min_sq):
    renders, frames, index = vc.score_case(size)
    bad = index.copy()
    bad[2], bad[5] = -1, len(frames)                     # NaN / -1 rows among good ones
    for idx in (index, bad):
        dev = metrics.gradient_scores(renders, frames, idx, red, render_min_sq, device="cuda")
        assert same(dev, metrics.gradient_scores(renders, frames, idx, red, render_min_sq))
    assert np.isnan(dev[0][[2, 5]]).all() and (dev[2][[2, 5]] == -1).all()


def _raw_scores(renders, grads, index, T, stream, fill):
    """bp_gradient_scores into output rows pre-filled with ``fill`` (dirty buffers), on ``stream``."""
    P, H, W = renders.shape[:3]
    d_sum = torch.full((P,), fill, dtype=torch.int64, device="cuda")
    d_count = torch.full((P,), fill, dtype=torch.int32, device="cuda")
    d_score = torch.full((P,), float(fill), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().bp_gradient_scores(_lib.ptr(renders), _lib.ptr(grads), _lib.ptr(index), P, T, H, W, 0, vc.SCENE_MIN_SQ,
                                             _lib.ptr(d_sum), _lib.ptr(d_count), _lib.ptr(d_score), stream.cuda_stream))
    return d_score, d_sum, d_count


@pytest.mark.parametrize("size", [(48, 64), (70, 130)])
def test_dirty_buffers_and_a_caller_stream(size):
    renders, frames, index = vc.score_case(size)
    want = metrics.gradient_scores(renders, frames, index, 0, vc.SCENE_MIN_SQ)
    grads_h, mags_h = metrics.image_gradients(frames)
    side = torch.cuda.Stream()
    d_renders, d_index = torch.from_numpy(renders).cuda(), torch.from_numpy(index).cuda()
    d_frames = torch.from_numpy(frames).cuda()
    T, H, W = frames.shape[:3]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_grads = torch.full((T, H, W, 2), 7.0, dtype=torch.float32, device="cuda")
        d_mags = torch.full((T, H, W), 7.0, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().bp_image_gradients(_lib.ptr(d_frames), T, H, W, 0, vc.SCENE_MIN_SQ, _lib.ptr(d_grads), _lib.ptr(d_mags),
                                                 side.cuda_stream))
        first = _raw_scores(d_renders, d_grads, d_index, T, side, 123456789)
        second = _raw_scores(d_renders, d_grads, d_index, T, side, -5)
    side.synchronize()
    assert same((d_grads.cpu().numpy(), d_mags.cpu().numpy()), (grads_h, mags_h))
    for got in (first, second):
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy().view(np.uint64), got[2].cpu().numpy()), want)
    assert _lib.lib().bp_gradient_scores(None, None, None, 0, 2, H, W, 0, 25, None, None, None, None) == 0      # P = 0


@pytest.mark.parametrize("textured", [False, True])
def test_verify_poses_equal_host(textured):
    size = (48, 64)
    pool0, frame0 = vc.disc_scene(0, size)
    pool1, frame1 = vc.disc_scene(1, size)
    poses = np.concatenate([pool0[:4], pool1[:4]])[[0, 4, 1, 5, 2, 6, 3, 7]]
    index = np.array([0, 1, 0, 1, 0, 1, 0, 1], np.int32)
    frames = np.concatenate([frame0, frame1])
    v, f, colors = vc.colored_mesh()
    kw = {}
    if textured:
        rng = np.random.default_rng(5)
        kw = {"uv": rng.uniform(0, 1, (len(f), 3, 2)), "texture": rng.integers(0, 256, (32, 16, 3), dtype=np.uint8)}
    K = rc.camera(size)
    want = metrics.verify_poses(poses, v, f, colors, K, frames, index, **kw)
    assert want[2].min() > 0
    for chunk in (0, 3):
        assert same(metrics.verify_poses(poses, v, f, colors, K, frames, index, device="cuda", chunk=chunk, **kw), want)


@pytest.mark.parametrize("seed", vc.DISC_SEEDS)
@pytest.mark.parametrize("size", vc.DISC_SIZES)
def test_true_pose_wins_with_the_host_scores(size, seed):
    pool, frame = vc.disc_scene(seed, size)
    v, f, colors = vc.colored_mesh()
    index = np.zeros(len(pool), np.int32)
    dev = metrics.verify_poses(pool, v, f, colors, rc.camera(size), frame, index, device="cuda")
    assert same(dev, metrics.verify_poses(pool, v, f, colors, rc.camera(size), frame, index))
    assert int(np.argmax(dev[0])) == 0


def _evaluate(outdir, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--synthetic", "4", "--sp", "--outdir", str(outdir),
                        "--candidates", "3", "--all_instances"] + list(flags), capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("Pose verification")]
    assert len(line) == 1, r.stdout
    return open(os.path.join(str(outdir), "Betapose-results.json")).read(), line[0]


@pytest.mark.parametrize("tail", [(), ("--device_pnp",)])
def test_evaluate_verify_host_and_device_scoring_agree(tmp_path, tail):
    dev_json, dev_line = _evaluate(tmp_path / "dev", "--verify", *tail)
    host_json, host_line = _evaluate(tmp_path / "host", "--verify", "host", *tail)
    assert dev_json == host_json and dev_line == host_line
    print(dev_line)
    assert len(json.loads(dev_json)) > 0
