#!/usr/bin/env python3
"""Occlusion-LineMod harness -- counterpart of the reference's ``occlusion_betapose_evaluate.py`` (run as in
``occlusion.sh``: ``--nClasses 50 --indir ... --outdir ... --sp --profile --conf 0.9 --obj_id N``).

    python occlusion_evaluate.py --indir <seq02/rgb> --outdir <out> --obj_id 5            # one object, as the reference
    python occlusion_evaluate.py --indir <seq02/rgb> --outdir <out> --obj_ids 1,5,6,8,9,10,11,12
    python -m torch.distributed.run --nproc-per-node 8 occlusion_evaluate.py --obj_ids ...   # units sharded over GPUs
    python occlusion_evaluate.py ... --obj_ids 1,5,6 --shared_detector yolo-linemod.cfg,linemod.weights   # one detector pass per frame

The reference evaluates ONE object per process: eight runs over the same 1214 frames of sequence 02, each decoding
every frame again and loading one detector + one key-point net (occlusion_betapose_evaluate.py:89-90,131-139).  With
``--obj_ids`` the unit of work is a (frame, object) pair: every object's two weight sets stay resident in
HBM (8 x 1.2 GB of 288 GB), a frame is decoded once and handed to every object's graph, units are sharded
``u % world`` over the ranks (u = frame * n_objects + object), the 316-float records are gathered per unit, and rank 0
prints the reference's three numbers per object -- ADD accuracy, 2-D reprojection accuracy at 20 px with the
``--left_keypoints`` best key points, IoU (occlusion_betapose_evaluate.py:204-260) -- and writes one
``obj_XX/Betapose-results.json`` per object.  Per object the results equal a single-object run of that object.

``--shared_detector CFG[,WEIGHTS]`` replaces the per-object detectors by ONE multi-class detector: a frame is resized
and detected once, the best box of each object's class (``--class_map``) feeds that object's key-point chain in the same
graph (``pipeline.ScenePipeline``).  Whole frames are then sharded ``f % world``; units, records, gather and output are
the same.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import evaluate  # noqa: E402


def main():
    if "--occlusion" not in sys.argv:
        sys.argv.append("--occlusion")
    from betapose_amd.opt import class_map, id_list, parse_args, shared_detector_arg
    args = parse_args()
    if not args.obj_ids:
        return evaluate.main()          # the reference's own protocol: one object per run (--candidates works there)
    if args.verify and not (int(args.candidates) and args.all_instances):
        raise SystemExit("--verify needs --candidates C --all_instances: it chooses among the instance poses of a frame")
    if args.all_instances and not int(args.candidates):
        raise SystemExit("--all_instances needs --candidates C: the instances are the merged poses of a frame's candidate boxes")
    if int(args.candidates):
        if args.pnp_ransac is not None:
            raise SystemExit("--candidates cannot be combined with --pnp_ransac: the candidate pose tail has no RANSAC variant yet")
        if args.shared_detector:
            raise SystemExit("--candidates cannot be combined with --shared_detector: candidates are boxes of ONE object's detector")
        raise SystemExit("--candidates: the multi-object runner of this harness has no candidate mode yet; "
                         "run one object at a time (--obj_id N instead of --obj_ids)")

    import torch
    from betapose_amd import _lib, dist as bpd, metrics, synth
    from betapose_amd.darknet import Darknet
    from betapose_amd.frame_loader import FrameLoader
    from betapose_amd.kpd import ALLPATHS, FastPoseHIP
    from betapose_amd.pipeline import POSE_DOUBLES, MultiObjectRunner, finish_pose_record, finish_record
    from betapose_amd.pPose_nms import write_json
    from betapose_amd.weights import fastpose_stream_from_state_dict, load_kpd_pkl, read_darknet_weights

    _lib.require_gpu()
    bpd.limit_host_threads()
    rank, world, local = bpd.init_from_env()
    obj_ids = id_list(args.obj_ids)
    symmetric = set(id_list(args.symmetric_ids))
    assert len(obj_ids) == len(set(obj_ids)) and obj_ids, "--obj_ids: distinct object ids"
    K = len(obj_ids)
    left_number = args.left_keypoints
    # --pnp_ransac [PX]: the RANSAC variant (100 trials, confidence 0.99: ops.solve_pnp_ransac's defaults) in either tail
    ransac = (float(args.pnp_ransac), 100, 0.99) if args.pnp_ransac is not None else None
    os.makedirs(args.outputpath, exist_ok=True)
    if len(args.inputlist):
        im_names = [l.strip() for l in open(args.inputlist)]
    elif len(args.inputpath) and args.inputpath != '/':
        im_names = sorted(f for f in os.listdir(args.inputpath) if f.lower().endswith((".png", ".jpg")))
    else:
        raise IOError('Error: must contain either --indir/--list')
    n_units = len(im_names) * K
    print("Betapose begin running now.  Occlusion objects", obj_ids, "| %d frames -> %d (frame, object) units | "
          "key points for PnP: %d" % (len(im_names), n_units, left_number))

    shared = shared_detector_arg(args.shared_detector) if args.shared_detector else None
    if shared:
        from betapose_amd.cfg import parse_cfg
        from betapose_amd.pipeline import frame_sharded_owner
        class_of = class_map(args.class_map, obj_ids)
        frame_owner = frame_sharded_owner(K, world)
        print("shared detector %s | object -> class %s" % (shared[0], class_of))

    def owned(u):
        return (frame_owner(u) if shared else bpd.owner_of(u, world)) == rank
    my_objs = [o for oi, o in enumerate(obj_ids) if any(owned(f * K + oi) for f in range(min(len(im_names), world)))]
    if shared and my_objs:
        my_objs = list(obj_ids)        # a rank that owns a frame runs all of its objects
    my_frames = [f for f in range(len(im_names)) if any(owned(f * K + oi) for oi in range(K))]

    # ---- ground truth / models per object (rank 0 evaluates)
    gt = {}
    if rank == 0:
        for o in obj_ids:
            frames_gt, model, kp3d, diameter, cam = evaluate.load_sixd_gt(args.sixd_base, o, 2)
            gt[o] = (frames_gt, model, metrics.refine_keypoints(kp3d, 50) if len(kp3d) > 50 else kp3d, diameter, cam)

    # ---- weights: rank 0 reads every object's two streams, all ranks receive them, each builds the engines it needs
    engines = {}
    t0 = time.time()
    shared_det = None
    if shared:
        ys = None
        if rank == 0:
            if args.synth_weights:      # seeded synthetic weights for that cfg (the fixtures' detector seed)
                ys = synth.synth_yolo_stream(1, [b for b in parse_cfg(shared[0]) if b["type"] != "net"])
            elif shared[1] is None:
                raise IOError("--shared_detector %s: give CFG,WEIGHTS (or --synth_weights)" % shared[0])
            else:
                ys = read_darknet_weights(shared[1])[2]
        ys = bpd.broadcast_stream(ys)
        if my_objs:
            shared_det = Darknet(shared[0], reso=int(args.inp_dim), max_batch=1, device=local)
            shared_det.load_stream(ys).cuda()
            shared_det.set_precision(args.precision)
        del ys
    for o in obj_ids:
        ys = ks = None
        if rank == 0:
            if args.synth_weights and not args.yolo_weights:
                sy, sk = synth.object_seeds(o)
                ys = None if shared else synth.synth_yolo_stream(sy)
                ks = fastpose_stream_from_state_dict(synth.synth_fastpose_state_dict(sk, args.nClasses), args.nClasses)
            else:
                ys = None if shared else read_darknet_weights('models/yolo/{:02d}.weights'.format(o))[2]
                ks = fastpose_stream_from_state_dict(load_kpd_pkl('./exp/final_model/' + ALLPATHS[o] + '.pkl'), args.nClasses)
        ys, ks = (None if shared else bpd.broadcast_stream(ys)), bpd.broadcast_stream(ks)
        if shared:
            if o in my_objs:
                pose = FastPoseHIP.from_stream(ks, n_classes=args.nClasses, max_batch=1, device=local).cuda()
                pose.set_precision(args.precision)
                engines[o] = pose
        elif o in my_objs:
            det = Darknet("yolo/cfg/yolov3-single.cfg", reso=int(args.inp_dim), max_batch=1, device=local)
            det.load_stream(ys).cuda()
            pose = FastPoseHIP.from_stream(ks, n_classes=args.nClasses, max_batch=1, device=local).cuda()
            det.set_precision(args.precision)
            pose.set_precision(args.precision)
            engines[o] = (det, pose)
        del ys, ks
    print("rank %d: %d object engine pairs resident (%s), %.1f s" % (rank, len(engines), sorted(engines), time.time() - t0))

    # ---- --device_pnp: every rank solves its own units, so it needs the 3-D key points of the objects it runs
    solvers = None
    if args.device_pnp:
        solvers = {}
        for o in my_objs:
            kp3d = gt[o][2] if o in gt else evaluate.load_sixd_gt(args.sixd_base, o, 2)[2]
            solvers[o] = (metrics.refine_keypoints(kp3d, 50) if len(kp3d) > 50 else kp3d, synth.CAM_K, left_number, ransac)

    # ---- run this rank's units
    recs, poses = {}, {}

    def keep(u, rec, pose=None):
        recs[u] = rec
        if pose is not None:
            poses[u] = pose
    t_dev = time.time()
    if my_frames:
        threads = max(1, min(args.load_threads, (os.cpu_count() or 8) // max(1, world)))
        loader = FrameLoader([os.path.join(args.inputpath, im_names[f]) for f in my_frames], threads=threads,
                             depth=max(16, 2 * args.streams + threads))
        runner = MultiObjectRunner(engines, obj_ids, loader.height, loader.width, streams=args.streams,
                                   confidence=args.confidence, num_classes=args.num_classes, pose_solvers=solvers,
                                   shared_detector=(shared_det, class_of) if shared else None)
        runner.run(loader, my_frames, owned, keep)
        loader.close()
    t_dev = time.time() - t_dev
    mine = sorted(recs)
    print("rank %d: %d units over %d decoded frames, %.1f units/sec (%d in flight)" % (
        rank, len(mine), len(my_frames), len(mine) / max(t_dev, 1e-9), args.streams))
    mine_recs = np.stack([recs[u] for u in mine]) if mine else np.zeros((0, 316), np.float32)
    # whole frames per rank (shared detector): rank 0 holds the most, ceil(frames / world) frames of K units
    most = -(-len(im_names) // world) * K if shared else None
    allrec = bpd.gather_records(mine_recs, mine, n_units, max_local=most)
    allpose = None
    if args.device_pnp:   # the pose rows ride the same gather, each f64 as a pair of f32 bit patterns
        mine_poses = np.stack([poses[u] for u in mine]) if mine else np.zeros((0, POSE_DOUBLES), np.float64)
        allpose = bpd.gather_records(mine_poses.view(np.float32), mine, n_units, max_local=most)

    if rank == 0:
        drawn = []      # --save_img: every object's scored results, drawn into one image per frame at the end
        for oi, o in enumerate(obj_ids):
            frames_gt, model, kp3d, diameter, cam = gt[o]
            final_result = []
            for f, name in enumerate(im_names):
                if allpose is not None:
                    out = finish_pose_record(allrec[f * K + oi], np.ascontiguousarray(allpose[f * K + oi]).view(np.float64), name)
                else:
                    out = finish_record(allrec[f * K + oi], name, kp3d, synth.CAM_K, left_number, ransac=ransac)
                if out["boxes"] is not None:
                    final_result.append(out)
            odir = os.path.join(args.outputpath, "obj_%02d" % o)
            os.makedirs(odir, exist_ok=True)
            write_json(final_result, odir)
            sym = o in symmetric
            depth_inputs, m_ref = None, None
            if args.vsd or args.refine_depth is not None:
                depth_inputs = evaluate.load_depth_inputs(args.sixd_base, o, 2, final_result, frames_gt, cam)
            if args.refine_depth is not None:   # before any error: the lines below are those of the refined poses
                m_ref = evaluate.refine_scored_poses(o, final_result, frames_gt, model, depth_inputs, diameter,
                                                     torch.device("cuda", local), args.refine_depth,
                                                     match_instances=args.all_instances)
            m = metrics.evaluate_results(final_result, frames_gt, model, cam, diameter, 20.0, symmetric=sym,
                                         device=torch.device("cuda", local) if sym else None,
                                         match_instances=args.all_instances)
            print("Mean add accuracy for seq %02d is: %.3f" % (o, m["mean_add"]))
            if sym:
                print("Mean add-s accuracy for seq %02d is: %.3f" % (o, m["mean_adds"]))
            print("2d reprojection accuracy with leftkeypoints %d for seq %02d is: %.3f" % (left_number, o, m["mean_2d_acc"]))
            print("Mean IoU for seq %02d is: %.3f" % (o, m["mean_iou"]))
            if args.bop_metrics:
                evaluate.print_bop_metrics(args.sixd_base, o, final_result, frames_gt, model, cam, diameter,
                                           torch.device("cuda", local), match_instances=args.all_instances)
            if args.vsd and m_ref is not None:      # the refinement pass has scored the refined poses already
                print("Mean vsd recall for seq %02d is: %.3f" % (o, m_ref["ar_vsd"]))
            elif args.vsd:
                evaluate.print_vsd_metrics(args.sixd_base, o, 2, final_result, frames_gt, model, cam, diameter,
                                           torch.device("cuda", local), match_instances=args.all_instances,
                                           depth_inputs=depth_inputs)
            if args.save_img:
                drawn.append({"model": evaluate.render_model(args.sixd_base, o), "results": final_result, "gt": frames_gt})
        if args.save_img:
            from betapose_amd import renderer
            n = renderer.save_pose_images(drawn, args.inputpath, args.outputpath, synth.CAM_K, torch.device("cuda", local),
                                          all_instances=args.all_instances)
            print("Saved %d images to %s" % (n, os.path.join(args.outputpath, "vis")))
    bpd.finalize()


if __name__ == "__main__":
    main()
