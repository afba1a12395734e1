#!/usr/bin/env python3
"""Key-point designator -- the counterpart of the reference's ``1_keypoint_designator`` (PCL's 3-D SIFT on the z field,
without PCL and without its visualiser):

    python designate.py --model models/obj_01.ply --output kpmodels/obj_01.ply [--total_kp_number 50]
                        [--method sift|fps] [--min_scale 0.01 --n_octaves 10 --n_scales_per_octave 5 --min_contrast 0.2]
                        [--device cuda:0]

The model's vertices are voxel-gridded and searched octave by octave (betapose_amd/designate.py sift_keypoints; the
defaults are the reference's main.cpp), the key points found are thinned to --total_kp_number as the reference's
Model3D.refine would thin them, and the result is written as an ASCII .ply in the layout of the reference's
``assets/sifts``, which annotate.py and evaluate.py read.  --method fps takes --total_kp_number farthest points of the
vertices instead.  Without --device everything runs on the host twins; no GPU is needed.  DESIGN.md 3.9.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from betapose_amd import designate as D, metrics  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="Keypoint Designation")
    p.add_argument("--model", required=True, type=str, help="the object's mesh or point cloud (.ply)")
    p.add_argument("--output", required=True, type=str, help="the key-point file to write (.ply)")
    p.add_argument("--total_kp_number", default=50, type=int, help="Total number of keypoints to keep.")
    p.add_argument("--method", default="sift", choices=("sift", "fps"), help="3-D SIFT (the reference's) or farthest points")
    p.add_argument("--min_scale", default=0.01, type=float, help="sigma of the smallest scale")
    p.add_argument("--n_octaves", default=10, type=int, help="doublings of the scale")
    p.add_argument("--n_scales_per_octave", default=5, type=int, help="scales within an octave")
    p.add_argument("--min_contrast", default=0.2, type=float, help="smallest |DoG| of a key point")
    p.add_argument("--device", default=None, type=str, help="torch device of the kernels (default: the host twins)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    vertices = metrics.load_ply_vertices(args.model)
    sift_args = {}
    if args.method == "sift":
        sift_args = dict(min_scale=args.min_scale, n_octaves=args.n_octaves, n_scales_per_octave=args.n_scales_per_octave,
                         min_contrast=args.min_contrast)
    kp, info = D.designate(vertices, args.total_kp_number, args.method, device=args.device, return_info=True, **sift_args)
    print("# of points in the model are %d" % len(vertices))
    for o, n in enumerate(info["octave_sizes"]):
        print("# of points in octave %d are %d" % (o, n))
    print("# of %s points in the result are %d" % ("SIFT" if args.method == "sift" else "farthest", info["found"]))
    print("# of key points kept are %d" % info["kept"])
    if not len(kp):
        raise SystemExit("no key point found: lower --min_contrast or raise --min_scale to the mesh's unit")
    D.write_ply(args.output, kp)
    print("wrote %s" % args.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
