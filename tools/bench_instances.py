#!/usr/bin/env python3
"""A pose for every merged candidate (csrc/pose_tail_inst.hip): what the extra launch costs, synthetic
weights, one GPU.  One JSON line; ``--out FILE`` also writes it there (profiles/pose_instances_bench.json).  HIP events,
median of 20 after 5 warm-up rounds, the variants of each comparison alternating on one stream (the protocol of
tools/bench_candidates.py):

  * the instance launch alone (``bp_pose_instances_from_merged``) at C = 8 with m = 1 and m = 8 merged poses, next to
    one one-wave PnP launch (``bp_solve_pnp_batch``, one problem) -- m = 1 copies a row, m = 8 solves seven poses side
    by side, so the claim under test is that m = 8 costs about one PnP launch and not seven;
  * ``CandidatePipeline`` at C = 8 with the instance poses on and off, on the same frame.

    python tools/bench_instances.py [--out profiles/pose_instances_bench.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from betapose_amd import ops, synth  # noqa: E402
from betapose_amd.pipeline import CandidatePipeline  # noqa: E402
from tools.bench_candidates import CONF, NMS, REPS, WARM, alternate, engines  # noqa: E402

C8 = 8


def planted(m, left):
    """merged [1, 8, 152], info [1, 4], poses [1, 166] with m merged poses, each the projection of the key-point model under
    its own pose (scores random, so the pruning has work to do)."""
    rng = np.random.default_rng(7)
    kp3d = synth.synth_kp3d(50)
    merged = np.zeros((1, C8, 152), np.float32)
    for j in range(m):
        a = 0.1 * j
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Y = kp3d @ R.T + np.array([-0.3 + 0.08 * j, 0.02, 0.8])
        uv = Y @ synth.CAM_K.T
        row = merged[0, j]
        row[0] = np.array([j], np.int32).view(np.float32)[0]
        row[1] = 1.5
        row[2::3], row[3::3], row[4::3] = uv[:, 0] / uv[:, 2], uv[:, 1] / uv[:, 2], rng.uniform(0.4, 0.9, 50)
    info = np.array([[m, m, 0, 1]], np.int32)
    poses = np.zeros((1, 166), np.float64)
    poses[0, 1] = min(50, left)
    p2 = merged[0, 0, 2:].reshape(50, 3)[None, :, :2].astype(np.float64)
    return (torch.from_numpy(merged).cuda(), torch.from_numpy(info).cuda(), torch.from_numpy(poses).cuda(),
            torch.from_numpy(p2).cuda())


def launches(left):
    kp3d = synth.synth_kp3d(50)
    variants = {}
    for m in (1, C8):
        mg, info, poses, p2 = planted(m, left)
        variants["instances_m%d" % m] = (lambda mg=mg, info=info, poses=poses: ops.pose_instances(mg, info, poses, kp3d, synth.CAM_K, left))
    k3 = torch.from_numpy(kp3d).cuda()
    variants["one_pnp_launch"] = lambda: ops.solve_pnp_batch(k3, p2, synth.CAM_K)
    ms = alternate(variants)
    # the solved rows are real solutions (status 0), so the timed launch is the full solver
    mg, info, poses, _ = planted(C8, left)
    st = ops.pose_instances(mg, info, poses, kp3d, synth.CAM_K, left)[0, 1:, 0].cpu().numpy()
    return {"launch_ms": ms, "solved_rows_status": [int(s) for s in st],
            "m8_over_m1": round(ms["instances_m8"]["median"] / ms["instances_m1"]["median"], 3),
            "m8_over_one_pnp_launch": round(ms["instances_m8"]["median"] / ms["one_pnp_launch"]["median"], 3),
            "note": "the wrappers allocate their outputs inside the timed region, the same for every variant"}


def pipelines(left):
    det, pose = engines("bf16x3")
    frame = torch.from_numpy(synth.synth_frame(99)).cuda().unsqueeze(0)
    kp3d = synth.synth_kp3d(50)
    mk = lambda: CandidatePipeline(det, pose, 480, 640, candidates=C8, nms_conf=NMS, confidence=CONF, frames=frame)  # noqa: E731
    off = mk().set_pose_solver(kp3d, synth.CAM_K, left).prepare()
    on = mk().set_pose_solver(kp3d, synth.CAM_K, left, all_instances=True).prepare()
    ms = alternate({"instances_off": off.enqueue, "instances_on": on.enqueue})
    torch.cuda.synchronize()
    return {"frame_ms": ms, "graph_nodes": {"instances_off": off.kernel_count(), "instances_on": on.kernel_count()},
            "candidates_found_in_sample_frame": int(on.counts.cpu()[0]), "merged_poses_in_sample_frame": int(on.info.cpu()[1]),
            "on_minus_off_ms": round(ms["instances_on"]["median"] - ms["instances_off"]["median"], 4)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_instances.py needs a GPU")
    left = 10
    res = {"what": "one more launch at the end of the candidate frame graph solves every merged pose (pose_instances_kernel, one "
                   "wave64 workgroup per slot), one MI355X", "samples": REPS, "warmup": WARM, "left_number": left,
           "launch": launches(left), "pipeline_c8_bf16x3": pipelines(left)}
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
