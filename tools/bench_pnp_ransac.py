#!/usr/bin/env python3
"""Cost of the device RANSAC PnP (csrc/pnp_ransac.hip) on one GPU.  One JSON line; ``--out FILE`` also
writes it there (profiles/pnp_ransac_bench.json).  One process; HIP events around each call, median of 20 after a warm-up.

  a. ops.solve_pnp_ransac_batch at P = 1 and 28, n = 10 and 50, 100 trials, 40 % planted outliers (12 px);
     ops.solve_pnp_batch on the same problems as the yardstick of one iterative launch;
  b. the host bp_solve_pnp_ransac on the same problems, per problem, one thread;
  c. the pose tail on records (bp_pose_from_records / _ransac) at batch 1 and 28, left_number 50;
  d. StreamedRunner frames/s (f16, 3 streams, batch 28) with the host RANSAC tail and the device RANSAC tail
     (``--no-streamed`` leaves it out).

``--kernel-only`` runs (a) alone: the run to put under ``rocprofv3 --kernel-trace --stats``.

    python tools/bench_pnp_ransac.py [--out profiles/pnp_ransac_bench.json] [--kernel-only] [--no-streamed]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from scipy.spatial.transform import Rotation as Rot  # noqa: E402

import helpers  # noqa: E402
from betapose_amd import _lib, ops, synth  # noqa: E402
from betapose_amd.pipeline import FramePipeline, StreamedRunner, finish_pose_record, finish_record  # noqa: E402

KP3D, K = synth.synth_kp3d(50), synth.CAM_K
RANSAC = (12.0, 100, 0.99)
FRAME_DIAGONAL = 800.0     # random-weight key points are no projection of anything: see tests/test_gpu_pnp_ransac.py


def problems(P, n, share=0.4, seed=7):
    rng = np.random.default_rng(seed)
    P3 = KP3D[:n] * 3.0
    out = []
    for _ in range(P):
        R = Rot.from_rotvec(rng.normal(0, 0.9, 3)).as_matrix()
        t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 1.5)])
        uv = (P3 @ R.T + t) @ K.T
        uv = uv[:, :2] / uv[:, 2:] + rng.normal(0, 0.5, (n, 2))
        nb = int(round(share * n))
        bad = rng.choice(n, nb, replace=False)
        uv[bad] += rng.uniform(30, 120, (nb, 2)) * rng.choice([-1, 1], (nb, 2))
        out.append(uv)
    return P3, np.array(out)


def event_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(float(np.median(ts)), 4)


def solver_bench(res):
    for P in (1, 28):
        for n in (10, 50):
            P3, P2 = problems(P, n)
            p3, p2 = torch.from_numpy(P3).cuda(), torch.from_numpy(P2).cuda()
            nbytes = int(_lib.lib().bp_pnp_ransac_workspace_bytes(P, RANSAC[1]))
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            key = "P%d_n%d" % (P, n)
            res["ransac_batch_ms_" + key] = event_ms(lambda: ops.solve_pnp_ransac_batch(p3, p2, K, *RANSAC, workspace=ws))
            res["iterative_batch_ms_" + key] = event_ms(lambda: ops.solve_pnp_batch(p3, p2, K))
            st = ops.solve_pnp_ransac_batch(p3, p2, K, *RANSAC)[1].cpu().numpy()
            ts, solved = [], 0
            for _ in range(5):
                for p in range(P):
                    t = time.perf_counter()
                    try:
                        ops.solve_pnp_ransac(P3, P2[p], K, *RANSAC)
                        solved += 1
                    except _lib.BetaposeHipError:
                        pass
                    ts.append(time.perf_counter() - t)
            res["host_ransac_us_per_problem_" + key] = round(float(np.median(ts)) * 1e6, 1)
            res["solved_" + key] = [int((st == 0).sum()), solved // 5]


def engines(max_batch, mode):
    from betapose_amd.darknet import Darknet
    from betapose_amd.kpd import FastPoseHIP
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416, max_batch=max_batch).load_stream(helpers.yolo_stream()).cuda()
    pose = FastPoseHIP(helpers.kpd_state_dict(), n_classes=50, max_batch=max_batch).cuda()
    det.set_precision(mode)
    pose.set_precision(mode)
    return det, pose


def tail_bench(res):
    det, pose = engines(1, "bf16x3")
    pipe = FramePipeline(det, pose, 480, 640, batch=1)
    recs = np.stack([pipe.run(f)[0] for f in synth.synth_frames(28, 4321)])
    rs = (FRAME_DIAGONAL,) + RANSAC[1:]
    for B in (1, 28):
        r = torch.from_numpy(np.resize(recs, (B, recs.shape[1]))).cuda()
        res["tail_iterative_ms_batch%d" % B] = event_ms(lambda: ops.pose_from_records(r, KP3D, K, 50))
        res["tail_ransac_ms_batch%d" % B] = event_ms(lambda: ops.pose_from_records_ransac(r, KP3D, K, 50, *rs))


def streamed_fps(paths, mode, streams, batch):
    from betapose_amd.frame_loader import FrameLoader
    det, pose = engines(batch, mode)
    rs = (FRAME_DIAGONAL,) + RANSAC[1:]
    out = {}
    for name in ("host_ransac_tail", "device_ransac_tail"):
        dev = name == "device_ransac_tail"
        runner = StreamedRunner(det, pose, 480, 640, streams=streams, batch=batch,
                                pose_solver=(KP3D, K, 50, rs) if dev else None)
        names = [os.path.basename(p) for p in paths]
        results = []
        if dev:
            def on(i, rec, row):
                results.append(finish_pose_record(rec, row, names[i]))
        else:
            def on(i, rec):
                results.append(finish_record(rec, names[i], KP3D, K, 50, ransac=rs))
        for rep in range(2):                       # the first pass captures the graphs and warms the loader
            ld = FrameLoader(paths, threads=8, depth=max(16, 2 * streams * batch + 8))
            results.clear()
            t = time.perf_counter()
            n = runner.run(ld, on)
            dt = time.perf_counter() - t
            ld.close()
        assert n == len(paths) == len(results)
        out[name] = round(n / dt, 1)
        del runner
    return out


def main():
    res = {"what": "RANSAC PnP, hypotheses in parallel on one MI355X against the host loop", "reproj_err_px": RANSAC[0],
           "max_trials": RANSAC[1], "confidence": RANSAC[2], "outlier_share": 0.4}
    solver_bench(res)
    if "--kernel-only" not in sys.argv:
        tail_bench(res)
        if "--no-streamed" not in sys.argv:
            from PIL import Image
            with tempfile.TemporaryDirectory() as tmp:
                paths = []
                for i, fr in enumerate(synth.synth_frames(224, 777)):
                    p = os.path.join(tmp, "%04d.png" % i)
                    Image.fromarray(fr[:, :, ::-1].copy()).save(p, compress_level=1)
                    paths.append(p)
                res["streamed_fps_f16_s3_b28"] = streamed_fps(paths, "f16", 3, 28)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
