#!/usr/bin/env python3
"""Pose verification by gradient agreement next to the render it scores, on tools/bench_render_color.py's scene: P = 64
poses of bench_vsd.py's closed synthetic mesh (20 000 vertices, 39 996 triangles, about 100 x 100 px of a 640 x 480
image), one pose per image, against ONE frame (random 8 x 8 px blocks with the first pose pasted over them).  Timed in
one run on device-resident inputs with HIP events, median of 20 after 3 warm-up calls, minimum and maximum beside it:
bp_image_gradients (the frame), bp_gradient_scores (the 64 renders), the bp_render_color call that makes them,
metrics.verify_poses end to end (uploads, render, score, four rows back; wall clock), and the same scoring in eager
torch on the device: gray, two 5 x 5 conv2d Sobels over a reflect-padded image, normalise, mask, dot, sum.  The host
twins are timed on a few renders and scaled to P, and checked against the device.  ``early_out_blocks`` is the share of
the score kernel's blocks whose tile with halo is one gray and which leave before they touch the scene, counted here
from the renders.  ``score_bytes`` is what the kernel must move (the renders once, the scene gradients under the tiles
that stay) and ``score_share_of_copy_rate`` that traffic over the time against 6.29 TB/s.  One JSON line; ``--out FILE``
also writes it there (profiles/).

    python tools/bench_verify.py [--out profiles/verify_bench.json]
"""
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from betapose_amd import _lib, metrics  # noqa: E402
from bench_pose_metrics import poses  # noqa: E402
from bench_vsd import sphere_mesh  # noqa: E402

P, H, W = 64, 480, 640
HOST_RENDERS = 4
WARMUP, RUNS = 3, 20
COPY_RATE = 6.29e12
TILE_W, TILE_H = 64, 16                    # csrc/verify.hip VT_W, VT_H


def timed(call, stream):
    """(median, minimum, maximum) in ms of RUNS calls after WARMUP."""
    for _ in range(WARMUP):
        call()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def wall(call):
    for _ in range(WARMUP):
        call()
    ms = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def torch_scores(d_renders, d_frame, render_min_sq, scene_min_sq):
    """The scoring in eager torch: float gray, conv2d Sobels, float masks and sums (not bit-identical to the kernels)."""
    w = torch.tensor([4899.0, 9617.0, 1868.0], device=d_renders.device) / 16384.0
    d = torch.tensor([-1.0, -2.0, 0.0, 2.0, 1.0], device=d_renders.device)
    s = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device=d_renders.device)
    k = torch.stack([s[:, None] * d[None, :], d[:, None] * s[None, :]])[:, None]

    def unit(img, min_sq):
        gray = torch.floor(img.float() @ w + 0.5)[:, None]
        g = torch.nn.functional.conv2d(torch.nn.functional.pad(gray, (2, 2, 2, 2), mode="reflect"), k)
        m2 = (g * g).sum(1, keepdim=True)
        keep = m2 >= min_sq
        return torch.where(keep, g / (m2.sqrt() + 0.001), torch.zeros_like(g)), keep
    rn, keep = unit(d_renders, float(render_min_sq))
    sn, _ = unit(d_frame, float(scene_min_sq))
    dot = (rn * sn).sum(1).abs().sum((1, 2))
    return dot / (keep.sum((1, 2, 3)) + 1)


def main():
    _lib.require_gpu()
    torch.backends.cudnn.allow_tf32 = False             # the yardstick computes in full float32
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda:0")
    cam = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    K = np.ascontiguousarray(cam).reshape(9)
    rng = np.random.default_rng(0)
    gt = np.ascontiguousarray(poses(rng, P)[0][:, :3])
    v, f = sphere_mesh()
    v, f = np.ascontiguousarray(v), np.ascontiguousarray(f)
    colors = rng.integers(0, 256, size=(len(v), 3), dtype=np.uint8)
    light = np.zeros(3)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    bg = np.kron(rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8), np.ones((8, 8, 1), np.uint8))
    c0, z0, _ = metrics.render_color(gt[:1], v, f, colors, cam, (H, W), dev)
    frame = metrics.overlay(bg[None], c0, z0, 256, dev)
    index = np.zeros(P, np.int32)

    d_model, d_faces, d_cols = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(colors).to(dev)
    d_poses = torch.from_numpy(gt.reshape(P, 12)).to(dev)
    d_color = torch.zeros((P, H, W, 3), dtype=torch.uint8, device=dev)
    d_depth = torch.zeros((P, H, W), dtype=torch.float32, device=dev)
    d_skip = torch.empty(P, dtype=torch.int32, device=dev)
    d_frame, d_index = torch.from_numpy(frame).to(dev), torch.from_numpy(index).to(dev)
    d_grad = torch.empty((1, H, W, 2), dtype=torch.float32, device=dev)
    d_mag = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    d_sum = torch.empty(P, dtype=torch.int64, device=dev)
    d_count = torch.empty(P, dtype=torch.int32, device=dev)
    d_score = torch.empty(P, dtype=torch.float64, device=dev)

    def render():
        _lib.check(L.bp_render_color(_lib.ptr(d_model), len(v), _lib.ptr(d_faces), len(f), _lib.ptr(d_cols), _lib.ptr(d_poses), P,
                                     None, P, _lib.ptr(K), H, W, 0.0, 0.01, 0.5, _lib.ptr(light), 0, _lib.ptr(d_color),
                                     _lib.ptr(d_depth), _lib.ptr(d_skip), stream.cuda_stream))

    def gradients():
        _lib.check(L.bp_image_gradients(_lib.ptr(d_frame), 1, H, W, 0, metrics.VERIFY_SCENE_MIN_SQ, _lib.ptr(d_grad), _lib.ptr(d_mag),
                                        stream.cuda_stream))

    def scores():
        _lib.check(L.bp_gradient_scores(_lib.ptr(d_color), _lib.ptr(d_grad), _lib.ptr(d_index), P, 1, H, W, 0,
                                        metrics.VERIFY_RENDER_MIN_SQ, _lib.ptr(d_sum), _lib.ptr(d_count), _lib.ptr(d_score),
                                        stream.cuda_stream))

    t_render = timed(render, stream)
    t_grad = timed(gradients, stream)
    t_score = timed(scores, stream)
    got = (d_score.cpu().numpy(), d_sum.cpu().numpy().view(np.uint64), d_count.cpu().numpy())
    t_torch = timed(lambda: torch_scores(d_color, d_frame, metrics.VERIFY_RENDER_MIN_SQ, metrics.VERIFY_SCENE_MIN_SQ), stream)
    torch_got = torch_scores(d_color, d_frame, metrics.VERIFY_RENDER_MIN_SQ, metrics.VERIFY_SCENE_MIN_SQ).cpu().numpy()
    torch_cpu = torch_scores(d_color[:HOST_RENDERS].cpu(), d_frame.cpu(), metrics.VERIFY_RENDER_MIN_SQ,
                             metrics.VERIFY_SCENE_MIN_SQ).numpy()       # the same text on the CPU, a few renders
    worst = int(np.argmax(np.abs(torch_got - got[0])))
    t_e2e = wall(lambda: metrics.verify_poses(gt, v, f, colors, cam, frame, index, dev))
    e2e = metrics.verify_poses(gt, v, f, colors, cam, frame, index, dev)

    # tiles of the score kernel that are one gray with their halo (they leave before the scene is read)
    renders = d_color.cpu().numpy()
    r64 = renders.astype(np.int64)
    gray = (4899 * r64[..., 0] + 9617 * r64[..., 1] + 1868 * r64[..., 2] + 8192) >> 14
    tiles = stay = 0
    for y0 in range(0, H, TILE_H):
        for x0 in range(0, W, TILE_W):
            t = gray[:, max(y0 - 2, 0):y0 + TILE_H + 2, max(x0 - 2, 0):x0 + TILE_W + 2].reshape(P, -1)
            stay += int((t.min(1) != t.max(1)).sum())
            tiles += P
    score_bytes = P * H * W * 3 + stay * TILE_W * TILE_H * 8 + P * 20

    h = HOST_RENDERS
    t = time.perf_counter()
    host_grads = metrics.image_gradients(frame)
    host_grad_s = time.perf_counter() - t
    t = time.perf_counter()
    host = metrics.gradient_scores(renders[:h], host_grads[0], index[:h])
    host_score_s = (time.perf_counter() - t) * P / h
    r3 = lambda x: round(x, 3)
    same = lambda a, b: bool(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)))
    line = json.dumps({
        "metric": "verify", "date": datetime.date.today().isoformat(), "P": P, "n": len(v), "faces": len(f), "H": H, "W": W,
        "device": torch.cuda.get_device_name(dev), "warmup": WARMUP, "runs": RUNS,
        "image_gradients_ms": r3(t_grad[0]), "image_gradients_ms_min": r3(t_grad[1]), "image_gradients_ms_max": r3(t_grad[2]),
        "gradient_scores_ms": r3(t_score[0]), "gradient_scores_ms_min": r3(t_score[1]), "gradient_scores_ms_max": r3(t_score[2]),
        "render_color_ms": r3(t_render[0]), "render_color_ms_min": r3(t_render[1]), "render_color_ms_max": r3(t_render[2]),
        "verify_poses_ms": r3(t_e2e[0]), "verify_poses_ms_min": r3(t_e2e[1]), "verify_poses_ms_max": r3(t_e2e[2]),
        "torch_scores_ms": r3(t_torch[0]), "torch_scores_ms_min": r3(t_torch[1]), "torch_scores_ms_max": r3(t_torch[2]),
        "torch_to_kernel_ratio": r3(t_torch[0] / t_score[0]), "score_to_render_ratio": r3(t_score[0] / t_render[0]),
        "early_out_blocks": r3(1.0 - stay / tiles), "score_blocks": tiles,
        "score_bytes": int(score_bytes), "score_share_of_copy_rate": r3(score_bytes / (t_score[0] * 1e-3) / COPY_RATE),
        "host_renders_timed": h, "host_image_gradients_s": round(host_grad_s, 4), "host_gradient_scores_s_scaled": round(host_score_s, 4),
        "speedup_scores": round(host_score_s / (t_score[0] * 1e-3), 1),
        "kept_render_px_mean": float(got[2].mean()), "best_pose": int(np.argmax(got[0])),
        "torch_max_abs_score_difference": float(np.abs(torch_got - got[0]).max()), "torch_worst_pose": worst,
        "torch_score_there": float(torch_got[worst]), "kernel_score_there": float(got[0][worst]),
        "torch_cpu_max_abs_score_difference": float(np.abs(torch_cpu - got[0][:HOST_RENDERS]).max()),
        "torch_device_vs_cpu_max_abs_difference": float(np.abs(torch_cpu - torch_got[:HOST_RENDERS]).max()),
        "gradients_byte_identical": same(d_grad.cpu().numpy(), host_grads[0]) and same(d_mag.cpu().numpy(), host_grads[1]),
        "scores_byte_identical": all(same(a[:h], b) for a, b in zip(got, host)),
        "verify_poses_equals_calls": all(same(a, b) for a, b in zip(e2e[:3], got))})
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
