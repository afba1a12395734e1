#!/usr/bin/env python3
"""Key-point annotator -- the counterpart of the reference's ``2_keypoint_annotator/annotate_keypoint.py`` with the same
options (its opt.py):

    python annotate.py --obj_id 1 --sixd_base <SIXD tree> --output_base <out>/ [--total_kp_number 50] [--train_split 180]
                       [--visibility] [--depth] [--reference_labels] [--device cuda:0]

Every frame of sequence ``obj_id`` under ``<sixd_base>/test`` that holds the object is annotated with the projections of
the designated key points (``kpmodels/obj_XX.ply``, thinned to --total_kp_number as the reference's Model3D.refine does)
and written in the reference's layout to ``<output_base><obj_id %02d>`` (betapose_amd/annotate.py write_annotations).
--visibility renders the object's mesh at every pose and marks the key points it hides from itself; --depth also tests
them against the sequence's depth images; --reference_labels writes the reference's box-to-box rescaled labels instead
of the true projections.  Without --device everything runs on the host twins; no GPU is needed.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from betapose_amd import annotate as A, metrics, sixd, synth  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="Keypoint Annotation")
    p.add_argument("--expID", default="default", type=str, help="Experiment ID")
    p.add_argument("--obj_id", default=1, type=int,
                   help="Object ID to annotate. Its sequence may hold other objects too (synthesize.py --models --seq N): only "
                        "the rows of this object are annotated.")
    p.add_argument("--total_kp_number", default=50, type=int, help="Total number of keypoints to annotate.")
    p.add_argument("--train_split", default=180, type=int, help="Select this number to train and others to test.")
    p.add_argument("--output_base", default="./kp_dataset/", type=str, help="Output base address.")
    p.add_argument("--sixd_base", default="./hinterstoisser", type=str,
                   help="Base of LineMod dataset, including models and designated keypoints dataset.")
    p.add_argument("--visibility", action="store_true", help="render the mesh and mark self-occluded key points")
    p.add_argument("--depth", action="store_true", help="also test the key points against the sequence's depth images")
    p.add_argument("--reference_labels", action="store_true", help="write the reference's box-to-box rescaled labels")
    p.add_argument("--device", default=None, type=str, help="torch device of the kernels (default: the host twins)")
    p.add_argument("--seed", default=0, type=int, help="seed of the train / eval split")
    return p


def load_bench(base, obj_id, total_kp, want_faces, load_depth):
    """load_sixd's benchmark of sequence ``obj_id`` with the object's mesh and its thinned key points attached, in
    metres: ``(bench, kp3d, faces or None, (H, W))``."""
    import yaml
    bench = sixd.load_sixd(base, obj_id, load_depth=load_depth)
    size = (480, 640)
    if os.path.exists(os.path.join(base, "camera.yml")):
        cam = yaml.safe_load(open(os.path.join(base, "camera.yml")))
        size = (int(cam.get("height", 480)), int(cam.get("width", 640)))
    else:
        bench.cam = np.array(synth.CAM_K, dtype=np.float64)     # the reference annotator's hard-wired LineMod camera
    name = "%02d" % obj_id
    path = os.path.join(base, "models", "obj_%s.ply" % name)
    model, faces = metrics.Model3D(), None
    if want_faces:
        v, faces = metrics.load_ply_mesh(path)
        model.vertices = v * bench.scale_to_meters
    else:
        model.load(path, scale=bench.scale_to_meters)
    bench.models[name] = model
    kp = metrics.Model3D()
    kp.load(os.path.join(base, "kpmodels", "obj_%s.ply" % name), scale=1.0)
    kp.refine(total_kp)                                         # (in millimetres, where its 100.0 start value is meant)
    bench.kpmodels[name] = kp
    return bench, kp.vertices * bench.scale_to_meters, faces, size


def main(argv=None):
    args = build_parser().parse_args(argv)
    bench, kp3d, faces, size = load_bench(args.sixd_base, args.obj_id, args.total_kp_number, args.visibility, args.depth)
    outdir = args.output_base + "%02d" % args.obj_id
    ann = A.annotate_sequence(bench, args.obj_id, kp3d, faces=faces, use_depth=args.depth, reference=args.reference_labels,
                              device=args.device, size=size)
    N = len(ann["frames"])
    if args.train_split > N:
        raise SystemExit("--train_split %d exceeds the %d annotated frames" % (args.train_split, N))
    A.write_annotations(outdir, ann, args.train_split, args.seed, image_size=size)
    visible = ((ann["kp_flags"] & A.VISIBLE) == A.VISIBLE).sum(axis=1)
    fract = "%.3f" % ann["visib_fract"].mean() if "visib_fract" in ann and N else "n/a"
    print("annotated %d frames of object %02d into %s: %.2f of %d key points visible per frame, mean visib_fract %s"
          % (N, args.obj_id, outdir, visible.mean() if N else 0.0, len(kp3d), fract))
    return 0


if __name__ == "__main__":
    sys.exit(main())
