#!/usr/bin/env python3
"""Training-scene synthesiser: an annotated SIXD tree of rendered frames from nothing but a mesh.

    python synthesize.py --model obj_01.ply [--occluders a.ply,b.ply] --obj_id N --frames N --out TREE/
                         [--size 480x640] [--camera fx,fy,cx,cy] [--backgrounds DIR] [--min_visib .3] [--seed 0]
                         [--device cuda:0] [--training_set DIR] [--no_texture]
    python synthesize.py --models a.ply,b.ply,... --obj_ids 1,5,6 --frames N --out TREE/ [--seq N] [--class_map 1:0,5:1,6:2]
                         [--label_box full|visible] [--detector_set DIR] [--train_split N] [the options above]

The model (and the occluders) are SIXD model files: millimetres, per-vertex colours where they have them.  A file with
texture coordinates (``texture_u`` / ``texture_v`` per vertex or a face ``texcoord`` list) and a ``comment TextureFile
NAME`` is rendered with that PNG, found beside the PLY; --no_texture ignores it.  The object is
rendered at seeded random poses, partly hidden by one instance of every occluder, pasted over a procedural background
(or windows of the PNG photographs under --backgrounds) through a camera model, and written with a simulated depth
sensor's images as sequence ``obj_id`` of the tree ``--out`` -- the tree ``annotate.py --sixd_base TREE --visibility
--depth`` reads (betapose_amd/synth.py synthesize_scenes, write_scene_tree).  The key-point file
``kpmodels/obj_XX.ply`` is designate.py's to write.  --training_set also lays the frames out for train_kpd.py and
train_detector.py; it needs the annotator's output directory ``<training_set>/annot/<obj_id %02d>`` to exist.
Without --device everything runs on the host twins; no GPU is needed, and the files are the same bytes either way.

--models makes scenes of SEVERAL targets instead (synth.py synthesize_multi): every mesh is placed on its
own, an object that shows less than --min_visib of itself is left out of its scene, and sequence --seq (default: the
first of --obj_ids) of the tree gets every remaining object's row in ``gt.yml`` -- with its visible box, fraction and
pixel counts -- and an instance mask ``mask/NNNN.png``.  --detector_set also writes the shared detector's training set:
one Darknet line per object and frame (class = --class_map, default the position in --obj_ids; box = --label_box), the
images beside them, ``train.txt`` / ``eval.txt`` and the ``obj.data`` train_detector.py and detector_map.py take.
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
    p.add_argument("--model", default=None, type=str, help="the object's mesh (.ply, millimetres)")
    p.add_argument("--models", default=None, type=str, help="comma-separated meshes, every one a target (instead of --model)")
    p.add_argument("--obj_ids", default=None, type=str, help="with --models: comma-separated object ids, one per mesh")
    p.add_argument("--seq", default=None, type=int, help="with --models: the sequence to write (default: the first object id)")
    p.add_argument("--class_map", default=None, type=str, help="with --detector_set: obj_id:class,... (default: position in --obj_ids)")
    p.add_argument("--label_box", default="full", choices=("full", "visible"), help="with --detector_set: which box a label holds")
    p.add_argument("--detector_set", default=None, type=str, help="with --models: also write the shared detector's training set here")
    p.add_argument("--train_split", default=None, type=int, help="with --detector_set: frames for training (default: nine in ten)")
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
    p.add_argument("--no_texture", action="store_true", help="ignore a mesh's TextureFile: vertex colours only")
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


def load_meshes(ids, paths, args):
    """({obj_id: (vertices, faces, colours)} in millimetres as the tree stores them, the meshes in metres as the
    synthesiser takes them: with uv and the texture's pyramid where the PLY names a texture and --no_texture is off)."""
    meshes, metres = {}, []
    for oid, path in zip(ids, paths):
        v, f, c, uv, texture_file = metrics.load_ply_textured_mesh(path)
        meshes[oid] = (v, f, c)
        mesh = (v * 0.001, f, c)
        if texture_file is not None and uv is not None and not args.no_texture:
            if not os.path.isfile(texture_file):
                raise SystemExit("%s names the texture %s, which does not exist (--no_texture renders without it)" % (path, texture_file))
            mesh = synth.textured_mesh(mesh + (uv, metrics.load_texture(texture_file)), args.device)
        metres.append(mesh)
    return meshes, metres


def main_multi(args, K, size):
    """--models: scenes of several targets, their tree and (--detector_set) the shared detector's training set."""
    from betapose_amd import annotate as A
    paths = [p for p in args.models.split(",") if p]
    if not args.obj_ids:
        raise SystemExit("--models needs --obj_ids, one id per mesh")
    ids = [int(v) for v in args.obj_ids.split(",") if v]
    if len(ids) != len(paths) or len(set(ids)) != len(ids):
        raise SystemExit("--obj_ids must name each of the %d meshes of --models once" % len(paths))
    seq = ids[0] if args.seq is None else args.seq
    meshes, metres = load_meshes(ids, paths, args)
    bank = load_bank(args.backgrounds) if args.backgrounds else None
    kept = np.zeros(len(ids), np.int64)
    fract = []
    for first in range(0, args.frames, CHUNK):
        n = min(CHUNK, args.frames - first)
        scenes = synth.synthesize_multi(metres, K, size, n, args.seed, obj_ids=ids, min_visib=args.min_visib, backgrounds=bank,
                                        first_scene=first, device=args.device)
        synth.write_scene_tree(args.out, seq, scenes, meshes, K, 0.001, first_frame=first)
        kept += scenes["present"].sum(axis=0)
        fract += scenes["visib_fract"][scenes["present"]].tolist()
    print("synthesised %d scenes of objects %s into sequence %02d of %s: %s kept, mean visib_fract %.3f"
          % (args.frames, ",".join("%02d" % i for i in ids), seq, args.out,
             " ".join("%02d:%d" % (i, k) for i, k in zip(ids, kept)), float(np.mean(fract)) if fract else 0.0))
    if args.detector_set:
        class_of = {oid: c for c, oid in enumerate(ids)}
        if args.class_map:
            class_of = {int(a): int(b) for a, b in (pair.split(":") for pair in args.class_map.split(",") if pair)}
        split = args.frames - args.frames // 10 if args.train_split is None else args.train_split
        annot = os.path.join(args.detector_set, "annot")
        A.write_multi_labels(args.out, seq, annot, class_of, split, args.seed, args.label_box, size)
        lists = synth.export_detector_set(args.out, seq, annot, args.detector_set)
        print("detector set of %d classes: %s" % (len(class_of), lists["data"]))
    return 0


def main(argv=None):
    args = build_parser().parse_args(argv)
    if (args.model is None) == (args.models is None):
        raise SystemExit("give exactly one of --model (one target and its occluders) and --models (several targets)")
    H, W = (int(v) for v in args.size.lower().split("x"))
    K = camera_matrix(args.camera, (H, W))
    if args.models is not None:
        return main_multi(args, K, (H, W))
    paths = [args.model] + [p for p in args.occluders.split(",") if p]
    ids = [args.obj_id] + [i for i in range(1, len(paths) + 1) if i != args.obj_id][:len(paths) - 1]
    meshes, metres = load_meshes(ids, paths, args)
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
