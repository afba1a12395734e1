#!/usr/bin/env python3
"""Training-scene synthesiser: an annotated SIXD tree of rendered frames from nothing but a mesh.

    python synthesize.py --model obj_01.ply [--occluders a.ply,b.ply] --obj_id N --frames N --out TREE/
                         [--size 480x640] [--camera fx,fy,cx,cy] [--backgrounds DIR] [--min_visib .3] [--seed 0]
                         [--device cuda:0] [--training_set DIR]

The model (and the occluders) are SIXD model files: millimetres, per-vertex colours where they have them.  The object is
rendered at seeded random poses, partly hidden by one instance of every occluder, pasted over a procedural background
(or windows of the PNG photographs under --backgrounds) through a camera model, and written with a simulated depth
sensor's images as sequence ``obj_id`` of the tree ``--out`` -- the tree ``annotate.py --sixd_base TREE --visibility
--depth`` reads (betapose_amd/synth.py synthesize_scenes, write_scene_tree).  The key-point file
``kpmodels/obj_XX.ply`` is designate.py's to write.  --training_set also lays the frames out for train_kpd.py and
train_detector.py; it needs the annotator's output directory ``<training_set>/annot/<obj_id %02d>`` to exist.
Without --device everything runs on the host twins; no GPU is needed, and the files are the same bytes either way.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from betapose_amd import metrics, synth  # noqa: E402

CHUNK = 64      # scenes synthesised and written at a time


def build_parser():
    p = argparse.ArgumentParser(description="Training-scene synthesiser")
    p.add_argument("--model", required=True, type=str, help="the object's mesh (.ply, millimetres)")
    p.add_argument("--occluders", default="", type=str, help="comma-separated meshes that may hide the object")
    p.add_argument("--obj_id", default=1, type=int, help="object id (and sequence number) in the tree")
    p.add_argument("--frames", default=200, type=int, help="number of scenes")
    p.add_argument("--out", required=True, type=str, help="the SIXD tree to write")
    p.add_argument("--size", default="480x640", type=str, help="image size HxW")
    p.add_argument("--camera", default=None, type=str, help="fx,fy,cx,cy (default: the LineMod camera scaled to --size)")
    p.add_argument("--backgrounds", default=None, type=str, help="directory of PNG photographs of one size (default: procedural)")
    p.add_argument("--min_visib", default=0.3, type=float, help="smallest visible fraction of the object")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--device", default=None, type=str, help="torch device of the kernels (default: the host twins)")
    p.add_argument("--training_set", default=None, type=str, help="also export the loaders' layout from <DIR>/annot/<obj_id>")
    return p


def camera_matrix(text, size):
    H, W = size
    if text is None:
        K = np.array(synth.CAM_K, dtype=np.float64)
        K[0] *= W / 640.0
        K[1] *= H / 480.0
        return K
    fx, fy, cx, cy = (float(v) for v in text.split(","))
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def load_bank(folder):
    from betapose_amd.frame_loader import decode_png
    names = sorted(n for n in os.listdir(folder) if n.lower().endswith(".png"))
    if not names:
        raise SystemExit("--backgrounds %s holds no .png file" % folder)
    images = []
    for n in names:
        with open(os.path.join(folder, n), "rb") as f:
            images.append(decode_png(f.read()))
    if len({im.shape for im in images}) != 1:
        raise SystemExit("the photographs under --backgrounds must share one size")
    return np.stack(images)


def main(argv=None):
    args = build_parser().parse_args(argv)
    H, W = (int(v) for v in args.size.lower().split("x"))
    K = camera_matrix(args.camera, (H, W))
    paths = [args.model] + [p for p in args.occluders.split(",") if p]
    ids = [args.obj_id] + [i for i in range(1, len(paths) + 1) if i != args.obj_id][:len(paths) - 1]
    meshes = {oid: metrics.load_ply_colored_mesh(p) for oid, p in zip(ids, paths)}         # millimetres
    metres = [(meshes[oid][0] * 0.001, meshes[oid][1], meshes[oid][2]) for oid in ids]
    bank = load_bank(args.backgrounds) if args.backgrounds else None
    redraws = dropped = 0
    fract = []
    for first in range(0, args.frames, CHUNK):
        n = min(CHUNK, args.frames - first)
        scenes = synth.synthesize_scenes(metres[0], metres[1:], K, (H, W), n, args.seed, obj_ids=ids, min_visib=args.min_visib,
                                         backgrounds=bank, first_scene=first, device=args.device)
        synth.write_scene_tree(args.out, args.obj_id, scenes, meshes, K, 0.001, first_frame=first)
        redraws += int(scenes["redraws"].sum())
        dropped += int((~scenes["present"][:, 1:].all(axis=1)).sum()) if len(ids) > 1 else 0
        fract += scenes["visib_fract"].tolist()
    print("synthesised %d scenes of object %02d into %s: mean visib_fract %.3f, %d occluder redraws, %d scenes left without occluders"
          % (args.frames, args.obj_id, args.out, float(np.mean(fract)) if fract else 0.0, redraws, dropped))
    if args.training_set:
        annot = os.path.join(args.training_set, "annot", "%02d" % args.obj_id)
        if not os.path.isdir(annot):
            raise SystemExit("--training_set needs annotate.py's output under %s" % annot)
        synth.export_training_set(args.out, annot, args.training_set, seq=args.obj_id)
    return 0


if __name__ == "__main__":
    sys.exit(main())
