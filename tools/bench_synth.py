#!/usr/bin/env python3
"""What a batch of synthesised training scenes costs: 64 scenes at 640 x 480, bench_vsd.py's closed mesh (20 000
vertices, 39 996 triangles, 7.5 cm radius) as the target and two smaller copies of it as occluders, the LineMod camera.
Every stage is timed alone on device-resident data with HIP events (median of 20 after a warm-up, as
bench_render_color.py does): the renders (target in colour, two occluders ``into`` it, the target's depth alone), the
procedural background, compose, the sensor depth and the mask boxes.  compose is timed at the neutral camera, at
radius 2 without noise and at radius 2 with noise and feather (the full model, the row DESIGN.md 3.15 quotes); its
bytes moved (background, colour and frame bytes plus the f32 depth: 13 per pixel) are set against the 6.29 TB/s copy
rate that DESIGN.md 3.10 uses as the floor of the per-pixel kernels.  The host twins are timed on a few scenes and scaled to 64, and
checked against the device on those.  One JSON line; ``--out FILE`` also writes it there (profiles/).

    python tools/bench_synth.py [--out profiles/synth_bench.json]
"""
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from betapose_amd import _lib, annotate as A, metrics, synth  # noqa: E402
from bench_vsd import RADIUS, sphere_mesh, timed  # noqa: E402

P, H, W = 64, 480, 640
HOST_SCENES = 4
COPY_FLOOR_TBS = 6.29
SEED = 0


def main():
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    cam = np.array(synth.CAM_K, dtype=np.float64)
    K = np.ascontiguousarray(cam).reshape(9)
    rng = np.random.default_rng(0)
    v, f = sphere_mesh()
    meshes = [(v, f), (v * 0.6, f), (v * 0.4, f)]
    cols = [rng.integers(0, 256, size=(len(v), 3), dtype=np.uint8) for _ in meshes]
    tposes = synth.sample_poses(P, cam, (H, W), RADIUS, SEED, distance=(0.6, 1.2))
    oposes = synth.place_occluders(tposes, RADIUS, cam, (H, W), SEED, 2)
    light = np.zeros(3)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_mesh = [(up(m[0]), up(m[1]), up(c)) for m, c in zip(meshes, cols)]
    d_poses = [up(tposes.reshape(P, 12)), up(oposes[:, 0].reshape(P, 12)), up(oposes[:, 1].reshape(P, 12))]
    d_color = torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)
    d_depth = torch.empty((P, H, W), dtype=torch.float32, device=dev)
    d_md = torch.empty((P, H, W), dtype=torch.float32, device=dev)
    d_skip = torch.empty(P, dtype=torch.int32, device=dev)
    d_bg = torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)
    d_frames = torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)
    d_u16 = torch.empty((P, H, W), dtype=torch.int16, device=dev)
    d_boxes = torch.empty((P, 2, 4), dtype=torch.int32, device=dev)
    d_counts = torch.empty((P, 2), dtype=torch.int32, device=dev)
    d_index = torch.arange(P, dtype=torch.int32, device=dev)
    tables = {"neutral": synth.compose_params(P, feather=0),
              "blur2": synth.compose_params(P, feather=0, blur=2),
              "full": synth.compose_params(P, feather=1, blur=2, gain=(270, 250, 240), offset=(3, -4, 5), sigma=768)}
    sensor = synth.sensor_params(P, 512, 30, 128)

    def renders():
        for j, ((dv, df, dc), dp) in enumerate(zip(d_mesh, d_poses)):
            _lib.check(L.bp_render_color(_lib.ptr(dv), len(v), _lib.ptr(df), len(f), _lib.ptr(dc), _lib.ptr(dp), P, None, P,
                                         _lib.ptr(K), H, W, 0.0, 0.01, 0.5, _lib.ptr(light), int(j > 0), _lib.ptr(d_color),
                                         _lib.ptr(d_depth), _lib.ptr(d_skip), s))
        dv, df, _ = d_mesh[0]
        _lib.check(L.bp_render_depth(_lib.ptr(dv), len(v), _lib.ptr(df), len(f), _lib.ptr(d_poses[0]), P, _lib.ptr(K), H, W,
                                     0.0, 0.01, _lib.ptr(d_md), _lib.ptr(d_skip), s))

    def background():
        _lib.check(L.bp_synth_background(P, H, W, SEED, 0, _lib.ptr(d_bg), s))

    def compose(table):
        return lambda: _lib.check(L.bp_synth_compose(_lib.ptr(d_bg), _lib.ptr(d_color), _lib.ptr(d_depth), P, H, W,
                                                     _lib.ptr(table), SEED, 0, _lib.ptr(d_frames), s))

    def sensor_depth():
        _lib.check(L.bp_synth_sensor_depth(_lib.ptr(d_depth), P, H, W, 0.001, _lib.ptr(sensor), SEED, 0, _lib.ptr(d_u16), s))

    d_scene = torch.empty((P, H, W), dtype=torch.float32, device=dev)

    def masks():
        _lib.check(L.bp_mask_boxes(_lib.ptr(d_md), P, H, W, _lib.ptr(K), 0.0, _lib.ptr(d_scene), P, _lib.ptr(d_index),
                                   metrics.BOP_VSD_DELTA, _lib.ptr(d_boxes), _lib.ptr(d_counts), s))

    ms = {}
    ms["renders"], _ = timed(renders, stream)
    ms["background"], _ = timed(background, stream)
    for name, table in tables.items():
        ms["compose_" + name], _ = timed(compose(table), stream)
    ms["sensor_depth"], _ = timed(sensor_depth, stream)
    d_scene.copy_(d_u16.to(torch.int32).bitwise_and(0xFFFF).to(torch.float32) * 0.001)
    ms["masks"], _ = timed(masks, stream)
    got = {"background": d_bg[:HOST_SCENES].cpu().numpy(), "frames": d_frames[:HOST_SCENES].cpu().numpy(),
           "depth": d_u16[:HOST_SCENES].cpu().numpy().view(np.uint16)}
    color, depth = d_color[:HOST_SCENES].cpu().numpy(), d_depth[:HOST_SCENES].cpu().numpy()
    visib = (d_counts[:, 1].float() / d_counts[:, 0].clamp(min=1).float()).mean().item()

    h = HOST_SCENES
    host, same = {}, {}

    def host_timed(name, call, key=None):
        t = time.perf_counter()
        out = call()
        host[name] = round((time.perf_counter() - t) * P / h, 3)
        if key:
            same[key] = bool(np.array_equal(out, got[key]))
        return out
    bg = host_timed("background", lambda: synth.procedural_background(h, (H, W), SEED), "background")
    host_timed("compose_full", lambda: synth.compose(bg, color, depth, tables["full"][:h], SEED), "frames")
    host_timed("sensor_depth", lambda: synth.sensor_depth(depth, 0.001, sensor[:h], SEED), "depth")
    md = d_md[:h].cpu().numpy()
    host_timed("masks", lambda: A.mask_boxes(md, cam, A.scene_depth_from_u16(got["depth"], 0.001))[0])
    t = time.perf_counter()
    synth.synthesize_scenes((v, f, cols[0]), [(v * 0.6, f, cols[1]), (v * 0.4, f, cols[2])], cam, (H, W), P, SEED, radius=RADIUS,
                            distance=(0.6, 1.2), device=dev)
    whole_s = time.perf_counter() - t

    moved = P * H * W * 13
    line = json.dumps({
        "metric": "synth", "date": datetime.date.today().isoformat(), "scenes": P, "H": H, "W": W, "n": len(v), "faces": len(f),
        "occluders": 2, "device": torch.cuda.get_device_name(dev), "mean_visib_fract": round(visib, 3),
        "ms": {k: round(x, 3) for k, x in ms.items()},
        "compose_bytes_moved": moved,
        "compose_tb_per_s": {k[len("compose_"):]: round(moved / (x * 1e-3) / 1e12, 3) for k, x in ms.items() if k.startswith("compose_")},
        "compose_fraction_of_copy_floor": {k[len("compose_"):]: round(moved / (x * 1e-3) / 1e12 / COPY_FLOOR_TBS, 3)
                                           for k, x in ms.items() if k.startswith("compose_")},
        "host_scenes_timed": h, "host_s_scaled": host, "host_equals_device": same,
        "synthesize_scenes_device_s": round(whole_s, 3)})
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
