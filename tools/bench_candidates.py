#!/usr/bin/env python3
"""Candidate boxes per frame against the one-box frame chain, synthetic weights, one GPU.  One JSON line;
``--out FILE`` also writes it there (profiles/candidates_bench.json).  HIP events, median of 20 after 5 warm-up rounds,
the two variants of each comparison alternating on one stream (the protocol of tools/bench_scene.py):

  * ``CandidatePipeline`` at C = 1, 4, 8 against ``FramePipeline`` at batch 1 on the same frame, bf16x3 and f16;
  * the NMS select from the head tensors (``forward_select_nms``, C = 8) against ``forward_select`` -- both include the
    detector pass, so the figure of interest is their difference;
  * the candidate tail alone (``bp_pose_from_candidate_records``, n = 1, 4, 8) against ``bp_pose_from_records``.

    python tools/bench_candidates.py [--out profiles/candidates_bench.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from betapose_amd import cfg as C, ops, synth  # noqa: E402
from betapose_amd.darknet import Darknet  # noqa: E402
from betapose_amd.kpd import FastPoseHIP  # noqa: E402
from betapose_amd.pipeline import CandidatePipeline, FramePipeline  # noqa: E402

REPS, WARM, LEFT, NMS, CONF = 20, 5, 10, 0.6, 0.01
CANDS = (1, 4, 8)


def stats(ts):
    ts = np.asarray(ts)
    return {"median": round(float(np.median(ts)), 4), "min": round(float(ts.min()), 4), "max": round(float(ts.max()), 4),
            "spread": round(float(ts.max() - ts.min()), 4)}


def alternate(variants):
    """{name: fn} -> {name: stats of ms}: the variants take turns on the current stream, one event pair around each."""
    ts = {k: [] for k in variants}
    for i in range(WARM + REPS):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= WARM:
                ts[name].append(e0.elapsed_time(e1))
    return {k: stats(v) for k, v in ts.items()}


def engines(mode):
    blocks = C.parse_cfg_text(C.yolov3_single_cfg_text())
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416).load_stream(synth.synth_yolo_stream(1, blocks)).cuda()
    pose = FastPoseHIP(synth.synth_fastpose_state_dict(2), max_batch=max(CANDS)).cuda()
    det.set_precision(mode)
    pose.set_precision(mode)
    return det, pose


def pipelines(mode):
    det, pose = engines(mode)
    frame = torch.from_numpy(synth.synth_frame(99)).cuda().unsqueeze(0)
    kp3d = synth.synth_kp3d(50)
    fp = FramePipeline(det, pose, 480, 640, batch=1, confidence=CONF, frames=frame).set_pose_solver(kp3d, synth.CAM_K, LEFT).prepare()
    variants, nodes, found = {"frame_pipeline": fp.enqueue}, {"frame_pipeline": None}, {}
    cps = {}
    for c in CANDS:
        cp = CandidatePipeline(det, pose, 480, 640, candidates=c, nms_conf=NMS, confidence=CONF, frames=frame)
        cps[c] = cp.set_pose_solver(kp3d, synth.CAM_K, LEFT).prepare()
        variants["candidates_%d" % c] = cp.enqueue
    ms = alternate(variants)
    nodes["frame_pipeline"] = fp.kernel_count()
    for c, cp in cps.items():
        nodes["candidates_%d" % c] = cp.kernel_count()
        found["candidates_%d" % c] = int(cp.counts.cpu()[0])
    out = {"frame_ms": ms, "graph_nodes": nodes, "candidates_found_in_sample_frame": found}
    for c in CANDS:
        out["candidates_%d_over_frame_pipeline" % c] = round(ms["candidates_%d" % c]["median"] / ms["frame_pipeline"]["median"], 3)
    # the select alone: both variants run the detector, the difference is the select kernels'
    x = torch.rand((1, 3, 416, 416), device="cuda")
    sel = alternate({"forward_select": lambda: det.forward_select(x, confidence=CONF),
                     "forward_select_nms_8": lambda: det.forward_select_nms(x, 8, NMS, confidence=CONF)})
    out["detector_plus_select_ms"] = sel
    out["nms_select_minus_select_ms"] = round(sel["forward_select_nms_8"]["median"] - sel["forward_select"]["median"], 4)
    return out, cps[max(CANDS)]


def tails(cp):
    """The tail alone on the records the C = 8 pipeline just wrote (its valid rows repeated up to n)."""
    recs = cp.results.clone()
    n_valid = max(1, int(cp.counts.cpu()[0]))
    kp3d = synth.synth_kp3d(50)
    one = recs[:1].contiguous()
    variants = {"pose_from_records": lambda: ops.pose_from_records(one, kp3d, synth.CAM_K, LEFT)}
    for n in CANDS:
        r = recs[torch.arange(n, device=recs.device) % n_valid].unsqueeze(0).contiguous()
        cnt = torch.tensor([n], dtype=torch.int32, device=recs.device)
        variants["candidate_tail_n%d" % n] = (lambda r=r, cnt=cnt: ops.pose_from_candidate_records(r, cnt, kp3d, synth.CAM_K, LEFT))
    ms = alternate(variants)
    out = {"tail_ms": ms, "note": "the wrappers allocate their outputs inside the timed region, the same for every variant"}
    for n in CANDS:
        out["candidate_tail_n%d_over_pose_from_records" % n] = round(ms["candidate_tail_n%d" % n]["median"] / ms["pose_from_records"]["median"], 3)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_candidates.py needs a GPU")
    res = {"what": "CandidatePipeline (C box-NMS survivors, one key-point pass at batch C, candidate pose tail) against FramePipeline "
                   "at batch 1 on the same frame, one MI355X", "samples": REPS, "warmup": WARM, "nms_conf": NMS,
           "pose_tail": "device, left_number %d" % LEFT}
    for mode in ("bf16x3", "f16"):
        res[mode], cp8 = pipelines(mode)
        if mode == "bf16x3":
            res["tail"] = tails(cp8)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
