#!/usr/bin/env python3
"""The textured colour renderer next to bp_render_color on the same scene, tools/bench_render_color.py's: P = 64 poses of
bench_vsd.py's closed synthetic mesh (20 000 vertices, 39 996 triangles, about 100 x 100 px of a 640 x 480 image), one
pose per image, with a 2 048 x 2 048 texture wrapped round it (u along the longitude, v along the latitude; the seam's
faces carry u + 1).  Timed in one run on device-resident inputs with HIP events, median of 20 after 3 warm-up calls,
minimum and maximum beside it: bp_render_color_textured, bp_render_color (the yardstick), the textured call with
``levels = 1`` (mip=False), the textured call with a 1 x 1 texture (every fetch hits one texel: the arithmetic alone) and
bp_texture_mips.  Clear, transform and visibility are the same launches in all of them, so a difference between two calls
is a difference between their resolves.  The host twins are timed on a few poses (the pyramid whole) and scaled to P, and
checked against the device on those.  One JSON line; ``--out FILE`` also writes it there (profiles/).

    python tools/bench_render_texture.py [--out profiles/render_texture_bench.json]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from betapose_amd import _lib, metrics  # noqa: E402
from bench_pose_metrics import poses  # noqa: E402
from bench_vsd import NLAT, NLON, sphere_mesh  # noqa: E402

P, H, W = 64, 480, 640
WT = HT = 2048
HOST_POSES = 2
WARMUP, RUNS = 3, 20


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


def sphere_uv(faces):
    """[F, 3, 2]: u = longitude / 2 pi, v = 1 - latitude / pi of bench_vsd.sphere_mesh's vertices; a face that crosses
    the seam has 1 added to its small u (the wrap is repeat)."""
    ring, col = np.arange(NLAT * NLON) // NLON, np.arange(NLAT * NLON) % NLON
    uv = np.stack([col / NLON, 1.0 - (ring + 0.5) / NLAT], axis=1)[faces]
    seam = (uv[:, :, 0].max(axis=1) - uv[:, :, 0].min(axis=1)) > 0.5
    uv[seam, :, 0] += (uv[seam, :, 0] < 0.5)
    return np.ascontiguousarray(uv)


def texture():
    rng = np.random.default_rng(1)
    ys, xs = np.mgrid[0:HT, 0:WT]
    t = np.stack([xs * 255 // (WT - 1), ys * 255 // (HT - 1), ((xs // 8 + ys // 8) & 1) * 255], axis=-1).astype(np.int64)
    return np.clip(t + rng.integers(-20, 21, size=t.shape), 0, 255).astype(np.uint8)


def main():
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    cam = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    K = np.ascontiguousarray(cam).reshape(9)
    rng = np.random.default_rng(0)
    gt = np.ascontiguousarray(poses(rng, P)[0][:, :3])
    v, f = sphere_mesh()
    colors = rng.integers(0, 256, size=(len(v), 3), dtype=np.uint8)
    uv, tex = sphere_uv(f), texture()
    light = np.zeros(3)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    d_model, d_faces = torch.from_numpy(np.ascontiguousarray(v)).to(dev), torch.from_numpy(np.ascontiguousarray(f)).to(dev)
    d_cols, d_uv, d_tex = torch.from_numpy(colors).to(dev), torch.from_numpy(uv).to(dev), torch.from_numpy(tex).to(dev)
    d_poses = torch.from_numpy(gt.reshape(P, 12)).to(dev)
    d_color = torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)
    d_depth = torch.empty((P, H, W), dtype=torch.float32, device=dev)
    d_skip = torch.empty(P, dtype=torch.int32, device=dev)
    levels = metrics.texture_levels(WT, HT)
    d_mips = torch.empty(L.bp_texture_mips_bytes(WT, HT, levels) // 4, dtype=torch.int32, device=dev)
    one = metrics.texture_mips(tex[:1, :1].copy(), dev)

    def build():
        _lib.check(L.bp_texture_mips(_lib.ptr(d_tex), WT, HT, levels, _lib.ptr(d_mips), stream.cuda_stream))

    def textured(mips, wt, ht, lv):
        def call():
            _lib.check(L.bp_render_color_textured(_lib.ptr(d_model), len(v), _lib.ptr(d_faces), len(f), None, _lib.ptr(d_uv),
                                                  _lib.ptr(mips), wt, ht, lv, _lib.ptr(d_poses), P, None, P, _lib.ptr(K), H, W,
                                                  0.0, 0.01, 0.5, _lib.ptr(light), 0, _lib.ptr(d_color), _lib.ptr(d_depth),
                                                  _lib.ptr(d_skip), stream.cuda_stream))
        return call

    def color():
        _lib.check(L.bp_render_color(_lib.ptr(d_model), len(v), _lib.ptr(d_faces), len(f), _lib.ptr(d_cols), _lib.ptr(d_poses), P,
                                     None, P, _lib.ptr(K), H, W, 0.0, 0.01, 0.5, _lib.ptr(light), 0, _lib.ptr(d_color),
                                     _lib.ptr(d_depth), _lib.ptr(d_skip), stream.cuda_stream))

    t_build = timed(build, stream)
    t_color = timed(color, stream)
    covered = float((d_depth > 0).float().sum())
    t_base = timed(textured(d_mips, WT, HT, 1), stream)
    got_base = d_color[:HOST_POSES].cpu().numpy()
    t_one = timed(textured(one.data, 1, 1, 1), stream)
    t_tex = timed(textured(d_mips, WT, HT, levels), stream)
    got_color, got_depth = d_color[:HOST_POSES].cpu().numpy(), d_depth[:HOST_POSES].cpu().numpy()

    h = HOST_POSES
    t = time.perf_counter()
    host_mips = metrics.texture_mips(tex)
    host_mips_s = time.perf_counter() - t
    t = time.perf_counter()
    ref = metrics.render_color(gt[:h], v, f, None, cam, (H, W), uv=uv, texture=host_mips)
    host_tex_s = (time.perf_counter() - t) * P / h
    ref_base = metrics.render_color(gt[:h], v, f, None, cam, (H, W), uv=uv, texture=host_mips, mip=False)
    t = time.perf_counter()
    metrics.render_color(gt[:h], v, f, colors, cam, (H, W))
    host_color_s = (time.perf_counter() - t) * P / h
    r3 = lambda x: round(x, 3)
    extra_ns = lambda a: round((a[0] - t_color[0]) * 1e6 / covered, 3)     # ns per covered pixel over the vertex-colour call
    line = json.dumps({
        "metric": "render_texture", "P": P, "n": len(v), "faces": len(f), "H": H, "W": W, "Wt": WT, "Ht": HT, "levels": levels,
        "device": torch.cuda.get_device_name(dev), "covered_px": int(covered), "warmup": WARMUP, "runs": RUNS,
        "textured_ms": r3(t_tex[0]), "textured_ms_min": r3(t_tex[1]), "textured_ms_max": r3(t_tex[2]),
        "render_color_ms": r3(t_color[0]), "render_color_ms_min": r3(t_color[1]), "render_color_ms_max": r3(t_color[2]),
        "textured_to_color_ratio": r3(t_tex[0] / t_color[0]),
        "textured_base_level_ms": r3(t_base[0]), "textured_base_level_ms_min": r3(t_base[1]), "textured_base_level_ms_max": r3(t_base[2]),
        "textured_1x1_ms": r3(t_one[0]), "textured_1x1_ms_min": r3(t_one[1]), "textured_1x1_ms_max": r3(t_one[2]),
        "mips_ms": r3(t_build[0]), "mips_ms_min": r3(t_build[1]), "mips_ms_max": r3(t_build[2]),
        "extra_ns_per_covered_px": {"textured": extra_ns(t_tex), "base_level": extra_ns(t_base), "1x1": extra_ns(t_one)},
        "host_poses_timed": h, "host_textured_s_scaled": round(host_tex_s, 4), "host_render_color_s_scaled": round(host_color_s, 4),
        "host_mips_s": round(host_mips_s, 4), "speedup": round(host_tex_s / (t_tex[0] * 1e-3), 1),
        "mips_byte_identical": bool(np.array_equal(d_mips.cpu().numpy().view(np.uint32), host_mips.data)),
        "color_byte_identical": bool(np.array_equal(got_color, ref[0])),
        "base_level_byte_identical": bool(np.array_equal(got_base, ref_base[0])),
        "depth_bit_identical": bool(np.array_equal(got_depth.view(np.uint32), ref[1].view(np.uint32)))})
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
