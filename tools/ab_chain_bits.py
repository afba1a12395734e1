#!/usr/bin/env python3
"""Bit-level A/B of the three per-frame chains between two builds of the library (csrc/frame_chain.h holds what
``bp_pipeline``, ``bp_scene`` and ``bp_cands`` share; a refactor of it must not move a bit or a graph node).  No timings,
no fixture, fixed seeds, synthetic weights.  Needs a GPU.

    BP_LIB=/path/to/libA.so python tools/ab_chain_bits.py --out A.npz     # one process per library, never two in one
    BP_LIB=/path/to/libB.so python tools/ab_chain_bits.py --out B.npz
    python tools/ab_chain_bits.py --compare A.npz B.npz                   # exit 1 unless every array is equal as integers

``--out`` runs two frames through ``FramePipeline`` (solver off / iterative / RANSAC, and a fixed box), ``ScenePipeline``
with two objects (solver off / iterative / RANSAC) and ``CandidatePipeline`` with four candidates (solver off, on, on with
instance poses), each with and without the hipGraph, and stores every output array raw -- records, pose rows, counts,
merged poses, info words, instance rows -- plus ``kernel_count()``.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ab_pose_bits import compare  # noqa: E402

OBJS = [1, 5]
CLASS_OF = {o: o - 1 for o in OBJS}
LEFT, RANSAC, CANDS = 10, (8.0, 64, 0.99), 4
FRAME_SEEDS = (99, 100)


def dump():
    import torch
    from betapose_amd import cfg as C, synth
    from betapose_amd.darknet import Darknet
    from betapose_amd.kpd import FastPoseHIP
    from betapose_amd.pipeline import CandidatePipeline, FramePipeline, ScenePipeline
    from betapose_amd.weights import fastpose_stream_from_state_dict

    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416)
    det.blocks = C.parse_cfg_text(C.yolov3_single_cfg_text(classes=15))
    det.net_info = det.blocks[0]
    det.load_stream(synth.synth_yolo_stream(1, det.blocks)).cuda()
    nets = {}
    for o in OBJS:
        sd = synth.synth_fastpose_state_dict(synth.object_seeds(o)[1], 50)
        nets[o] = FastPoseHIP.from_stream(fastpose_stream_from_state_dict(sd, 50), n_classes=50, max_batch=CANDS).cuda()
    frames = [synth.synth_frame(s) for s in FRAME_SEEDS]
    solver = {o: (synth.synth_kp3d(50, seed=7 + o), synth.CAM_K, LEFT) for o in OBJS}
    out = {}

    def run(tag, chain, names):
        for i, f in enumerate(frames):
            chain.run(f)
            torch.cuda.synchronize()
            for n in names:
                out["%s/frame%d_%s" % (tag, i, n)] = getattr(chain, n).cpu().numpy()
        out["%s/nodes" % tag] = np.array([chain.kernel_count()], np.int32)

    for graph in (True, False):
        g = "graph" if graph else "eager"
        for mode in ("off", "iter", "ransac", "fixed_box"):
            fp = FramePipeline(det, nets[1], 480, 640, batch=1, confidence=0.01, use_graph=graph)
            if mode in ("iter", "ransac"):
                fp.set_pose_solver(*solver[1], ransac=RANSAC if mode == "ransac" else None)
            if mode == "fixed_box":
                fp.set_fixed_box([200.0, 120.0, 420.0, 380.0])
            run("pipeline_%s_%s" % (mode, g), fp, ["results"] + (["poses"] if fp.poses is not None else []))
        for mode in ("off", "iter", "ransac"):
            sp = ScenePipeline(det, nets, CLASS_OF, 480, 640, confidence=0.01, use_graph=graph)
            if mode != "off":
                for o in OBJS:
                    sp.set_pose_solver(o, *solver[o], ransac=RANSAC if mode == "ransac" else None)
            run("scene_%s_%s" % (mode, g), sp, ["results"] + (["poses"] if sp.poses is not None else []))
        for mode in ("off", "pose", "instances"):
            cp = CandidatePipeline(det, nets[1], 480, 640, candidates=CANDS, confidence=0.01, class_id=CLASS_OF[1],
                                   use_graph=graph)
            names = ["results", "counts"]
            if mode != "off":
                cp.set_pose_solver(*solver[1], all_instances=mode == "instances")
                names += ["poses", "merged", "info"] + (["inst_poses"] if mode == "instances" else [])
            run("cands_%s_%s" % (mode, g), cp, names)
    return out


if __name__ == "__main__":
    if "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        sys.exit(compare(sys.argv[i + 1], sys.argv[i + 2]))
    if "--out" not in sys.argv:
        sys.exit(__doc__)
    arrays = dump()
    np.savez(sys.argv[sys.argv.index("--out") + 1], **arrays)
    print("%d arrays (%s)" % (len(arrays), ", ".join(sorted({k.split("/")[0] for k in arrays}))))
