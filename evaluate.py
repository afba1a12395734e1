#!/usr/bin/env python3
"""LineMod single-object evaluation harness on the HIP engines -- the counterpart of the reference's
``betapose_evaluate.py`` (3_6Dpose_estimator/betapose_evaluate.py:86-266) with the same flags (betapose_amd/opt.py):

    python evaluate.py --nClasses 50 --indir <frames> --outdir <out> --sp [--profile] [--obj_id N]
    python evaluate.py --synthetic 16 --outdir /tmp/out [--fused]          # no LineMod needed
    python -m torch.distributed.run --nproc-per-node 8 evaluate.py --fused ...   # frames sharded over GPUs

Default = the reference's staged pipeline (ImageLoader -> DetectionLoader -> DetectionProcessor -> KPD main loop ->
DataWriter, threads + queues).  ``--fused`` = one hipGraph per frame (betapose_amd/pipeline.py), frames round-robined
over ranks, records gathered to rank 0.  Both write ``Betapose-results.json`` and, when LineMod ground truth is
available under --sixd_base, print the reference's three numbers (ADD accuracy, 2-D reprojection accuracy, IoU).
"""
from __future__ import annotations

import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from betapose_amd import dist as bpd, metrics, synth  # noqa: E402
from betapose_amd.opt import id_list, parse_args  # noqa: E402


def load_sixd_gt(base, obj_id, seq_id=None):
    """Minimal ``load_sixd`` (utils/sixd.py:60-111): camera, model, key-point model, per-frame GT of object ``obj_id``
    in sequence ``seq_id`` (LineMod: the object's own sequence; Occlusion-LineMod: always sequence 02, where every
    frame lists several objects -- occlusion_betapose_evaluate.py:204,218-220)."""
    import yaml
    seq = os.path.join(base, "test", "%02d" % (obj_id if seq_id is None else seq_id))
    gt = yaml.safe_load(open(os.path.join(seq, "gt.yml")))
    info = yaml.safe_load(open(os.path.join(base, "models", "models_info.yml")))
    frames = {}
    for nr, objs in gt.items():
        # LineMod looks at the frame's FIRST annotation only and skips the frame when that is another object
        # (betapose_evaluate.py:219-221); Occlusion-LineMod walks every annotation of the frame
        # (occlusion_betapose_evaluate.py:218-220)
        cand = objs if seq_id is not None else objs[:1]
        ent = []
        for o in cand:
            if o["obj_id"] == obj_id:
                pose = np.eye(4)
                pose[:3, :3] = np.array(o["cam_R_m2c"]).reshape(3, 3)
                pose[:3, 3] = np.array(o["cam_t_m2c"]).reshape(3) / 1000.0
                ent.append({"pose": pose, "bbox": list(o["obj_bb"])})
        frames[int(nr)] = ent
    model = metrics.load_ply_vertices(os.path.join(base, "models", "obj_%02d.ply" % obj_id)) / 1000.0
    kp = metrics.load_ply_vertices(os.path.join(base, "kpmodels", "obj_%02d.ply" % obj_id)) / 1000.0
    # camera of the 2-D reprojection metric: camera.yml when the dataset has one, identity otherwise
    # (utils/sixd.py:53-68 -- ``Benchmark.cam``); PnP always uses the hard-coded LineMod K (betapose_evaluate.py:59)
    cam = np.identity(3)
    if os.path.exists(os.path.join(base, "camera.yml")):
        c = yaml.safe_load(open(os.path.join(base, "camera.yml")))
        cam[0, 0], cam[0, 2], cam[1, 1], cam[1, 2] = c["fx"], c["cx"], c["fy"], c["cy"]
    # the reference indexes a list built in models_info.yml key order (sixd.py:72-76), which equals a lookup by
    # object id for the 1..N keys every SIXD dataset has
    return frames, model, kp, float(info[obj_id]["diameter"]), cam


def print_bop_metrics(base, obj_id, final_result, gt_frames, model_vertices, cam, diameter, device, match_instances=False):
    """--bop_metrics: the object's symmetry set from models_info.yml, MSSD / MSPD of the scored pairs on ``device``, and
    the two average-recall lines (the lines before them are computed as without the flag)."""
    m = metrics.evaluate_results(final_result, gt_frames, model_vertices, cam, diameter, device=device,
                                 symmetries=metrics.load_symmetries(base, obj_id),
                                 image_width=metrics.load_image_width(base), match_instances=match_instances)
    print("Mean mssd recall for seq %02d is: %.3f" % (obj_id, m["ar_mssd"]))
    print("Mean mspd recall for seq %02d is: %.3f" % (obj_id, m["ar_mspd"]))


def load_depth_inputs(base, obj_id, seq_id, final_result, gt_frames, cam):
    """What --vsd and --refine_depth read alike: the faces of the object's mesh, the depth images of the scored frames and
    the camera -- camera.yml's when the dataset has one, else the LineMod K PnP uses."""
    from betapose_amd import sixd
    _, faces = metrics.load_ply_mesh(os.path.join(base, "models", "obj_%02d.ply" % obj_id))
    seq = os.path.join(base, "test", "%02d" % (obj_id if seq_id is None else seq_id))
    depth_frames = {}
    for f in final_result:
        nr = int(os.path.basename(f["imgname"])[0:-4])
        if nr in gt_frames and nr not in depth_frames:
            depth_frames[nr] = sixd.read_depth_png(os.path.join(seq, "depth", "%04d.png" % nr))
    K = cam if os.path.exists(os.path.join(base, "camera.yml")) else synth.CAM_K
    return faces, depth_frames, K


def print_vsd_metrics(base, obj_id, seq_id, final_result, gt_frames, model_vertices, cam, diameter, device,
                      match_instances=False, depth_inputs=None):
    """--vsd: VSD of the scored pairs on ``device`` and the average-recall line (``depth_inputs``: what load_depth_inputs
    returned when --refine_depth has read it already)."""
    faces, depth_frames, K = depth_inputs or load_depth_inputs(base, obj_id, seq_id, final_result, gt_frames, cam)
    m = metrics.evaluate_results(final_result, gt_frames, model_vertices, K, diameter, device=device, faces=faces,
                                 depth_frames=depth_frames, match_instances=match_instances)
    print("Mean vsd recall for seq %02d is: %.3f" % (obj_id, m["ar_vsd"]))


def refine_scored_poses(obj_id, final_result, gt_frames, model_vertices, depth_inputs, diameter, device, iterations,
                        match_instances=False):
    """--refine_depth: one evaluate_results pass with ``refine_depth`` set, on the camera of ``depth_inputs``.  It leaves
    the refined pose of every scored frame dict in cam_R / cam_t (the unrefined one under "pose_rgb"), so every later
    metric pass scores the refined poses; prints the counts line and returns the pass's metrics (VSD among them)."""
    faces, depth_frames, K = depth_inputs
    m = metrics.evaluate_results(final_result, gt_frames, model_vertices, K, diameter, device=device, faces=faces,
                                 depth_frames=depth_frames, match_instances=match_instances,
                                 refine_depth={"iterations": int(iterations)})
    print("Depth refinement for seq %02d: %d refined, %d rejected, %d unchanged, mean rms %.5f -> %.5f" % (
        obj_id, m["refined"], m["rejected"], m["unchanged"], m["mean_rms_first"], m["mean_rms_last"]))
    return m


def render_model(base, obj_id, kp3d=None):
    """What --save_img draws for an object: its coloured mesh in metres, or without a dataset a grey box around the key
    points."""
    from betapose_amd import renderer
    if base is None:
        return renderer.BoxModel(kp3d)
    model = metrics.Model3D()
    model.load_mesh(os.path.join(base, "models", "obj_%02d.ply" % obj_id), scale=0.001)
    return model


def save_images(args, obj_id, final_result, gt_frames, kp3d, cam_K, device):
    """--save_img: <outdir>/vis/<imgname>.png, the frame with the estimated pose's mesh at alpha 128, its 3-D box and the
    ground-truth box in green (betapose_amd/renderer.py save_pose_images), rendered on ``device`` a batch of frames at a
    time."""
    from betapose_amd import renderer
    t0 = time.time()
    model = render_model(None if gt_frames is None else args.sixd_base, obj_id, kp3d)
    n = renderer.save_pose_images([{"model": model, "results": final_result, "gt": gt_frames}], args.inputpath,
                                  args.outputpath, cam_K, device, all_instances=args.all_instances)
    print("Saved %d images to %s (%.1f frames/sec)" % (n, os.path.join(args.outputpath, "vis"), n / max(time.time() - t0, 1e-9)))


def verify_frame_poses(args, obj_id, final_result, gt_frames, kp3d, cam_K, device):
    """--verify: renderer.verify_results with the mesh --save_img draws (without a dataset: a grey box), on ``device`` or
    with ``--verify host`` by the host twin; prints the counts."""
    from betapose_amd import renderer
    model = render_model(None if gt_frames is None else args.sixd_base, obj_id, kp3d)
    scored, changed = renderer.verify_results(final_result, model, args.inputpath, cam_K,
                                              None if args.verify == "host" else device)
    print("Pose verification for seq %02d: %d frames scored, %d choices changed" % (obj_id, scored, changed))


def synthetic_depth_inputs(final_result, kp3d, cam_K, size, device):
    """--synthetic --vsd / --refine_depth: a closed loop that only shows the path runs.  The mesh is the bounding box of
    the synthetic key points, the ground truth is each frame's own estimated pose and its depth image is rendered from
    that pose."""
    lo, hi = np.min(kp3d, axis=0), np.max(kp3d, axis=0)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], dtype=np.float64)
    faces = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                      [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    gt_frames, depth_frames = {}, {}
    for f in final_result:
        if len(f["result"]) < 1:
            continue
        nr = int(os.path.basename(f["imgname"])[0:-4])
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = f["cam_R"], np.asarray(f["cam_t"])[:, 0]
        x1, y1, x2, y2 = np.asarray(f["result"][0]["bbox"]).tolist()
        gt_frames[nr] = [{"pose": pose, "bbox": [x1, y1, x2 - x1, y2 - y1]}]
        depth = metrics.render_depth(pose[None], v, faces, cam_K, size, device)[0][0]
        depth_frames[nr] = np.clip(np.round(depth.astype(np.float64) * 1000.0), 0, 65535).astype(np.uint16)
    diameter = float(np.linalg.norm(hi - lo)) * 1000.0
    return v, faces, gt_frames, depth_frames, diameter


def print_synthetic_vsd(obj_id, final_result, kp3d, cam_K, size, device, vsd=True, refine_iterations=None):
    """--synthetic --vsd: a frame whose pose puts the box in front of the camera scores 0 error and any other renders
    nothing and scores 1.  ``refine_iterations`` (--synthetic --refine_depth): the poses are first refined against those
    images -- they start at the poses the images were rendered from -- and the counts line and the accuracy lines of the
    refined poses are printed; the VSD line only with ``vsd``."""
    v, faces, gt_frames, depth_frames, diameter = synthetic_depth_inputs(final_result, kp3d, cam_K, size, device)
    if refine_iterations is not None:
        m = refine_scored_poses(obj_id, final_result, gt_frames, v, (faces, depth_frames, cam_K), diameter, device,
                                refine_iterations)
        print("Mean add accuracy for seq %02d is: %.3f" % (obj_id, m["mean_add"]))
        print("2d reprojection accuracy for seq %02d is: %.3f" % (obj_id, m["mean_2d_acc"]))
        print("Mean IoU for seq %02d is: %.3f" % (obj_id, m["mean_iou"]))
    else:
        m = metrics.evaluate_results(final_result, gt_frames, v, cam_K, diameter, device=device, faces=faces,
                                     depth_frames=depth_frames)
    if vsd:
        print("Mean vsd recall for seq %02d is: %.3f" % (obj_id, m["ar_vsd"]))


def main():
    args = parse_args()
    if args.verify and not (int(args.candidates) and args.all_instances):      # (before anything needs the GPU)
        raise SystemExit("--verify needs --candidates C --all_instances: it chooses among the instance poses of a frame")
    import torch
    from betapose_amd import _lib
    from betapose_amd.darknet import Darknet
    from betapose_amd.kpd import ALLPATHS, FastPoseHIP
    from betapose_amd.pPose_nms import write_json
    from betapose_amd.weights import fastpose_stream_from_state_dict, load_kpd_pkl, read_darknet_weights

    _lib.require_gpu()
    bpd.limit_host_threads()
    rank, world, local = bpd.init_from_env()
    obj_id = args.obj_id
    # key points handed to PnP: all 50 on LineMod (betapose_evaluate.py:139), the --left_keypoints best on Occlusion
    left_number = args.left_keypoints if args.occlusion else 50
    # --pnp_ransac [PX]: the RANSAC variant (100 trials, confidence 0.99: ops.solve_pnp_ransac's defaults) in either tail
    ransac = (float(args.pnp_ransac), 100, 0.99) if args.pnp_ransac is not None else None
    pixel_thresh = 20.0 if args.occlusion else 5.0          # occlusion_betapose_evaluate.py:255 vs betapose_evaluate.py:257
    C_ = int(args.candidates)
    if args.all_instances and not C_:
        raise SystemExit("--all_instances needs --candidates C: the instances are the merged poses of a frame's candidate boxes")
    if C_:
        from betapose_amd._lib import MAX_CANDIDATES
        if not 1 <= C_ <= MAX_CANDIDATES:
            raise SystemExit("--candidates takes 1 to %d candidate boxes per frame, not %d" % (MAX_CANDIDATES, C_))
        if ransac is not None:
            raise SystemExit("--candidates cannot be combined with --pnp_ransac: the candidate pose tail has no RANSAC variant yet")
        if getattr(args, "shared_detector", ""):
            raise SystemExit("--candidates cannot be combined with --shared_detector: candidates are boxes of ONE object's detector")
        args.fused = True   # the candidate chain exists in the fused frame graph only
        if max(1, args.detbatch) != 1:
            raise SystemExit("--candidates runs one frame per launch: leave --detbatch at 1")
    print("Betapose begin running now.  Test object", obj_id, "| key points for PnP:", left_number)
    os.makedirs(args.outputpath, exist_ok=True)

    # ---- inputs
    gt_frames, model_vertices, diameter, metric_cam = None, None, None, None
    if args.synthetic:
        from PIL import Image
        args.inputpath = tempfile.mkdtemp(prefix="bp_frames_")
        im_names = []
        if rank == 0 or True:
            for i, fr in enumerate(synth.synth_frames(args.synthetic, 1234)):
                name = "%04d.png" % i
                Image.fromarray(fr[:, :, ::-1].copy()).save(os.path.join(args.inputpath, name))
                im_names.append(name)
                synth_size = fr.shape[:2]
        cam_K, kp3d = synth.CAM_K, synth.synth_kp3d(50)
    else:
        if len(args.inputlist):
            im_names = [l.strip() for l in open(args.inputlist)]
        elif len(args.inputpath) and args.inputpath != '/':
            im_names = sorted(f for f in os.listdir(args.inputpath) if f.lower().endswith((".png", ".jpg")))
        else:
            raise IOError('Error: must contain either --indir/--list')
        cam_K = synth.CAM_K
        gt_frames, model_vertices, kp3d, diameter, metric_cam = load_sixd_gt(args.sixd_base, obj_id, 2 if args.occlusion else None)
        kp3d = metrics.refine_keypoints(kp3d, 50) if len(kp3d) > 50 else kp3d

    # ---- weights: rank 0 reads the files, the fp32 streams are broadcast (RCCL)
    ys = ks = None
    if rank == 0:
        if (args.synthetic or args.synth_weights) and not args.yolo_weights:
            sy, sk = synth.object_seeds(obj_id) if not args.synthetic else (1, 2)
            ys = synth.synth_yolo_stream(sy)
            ks = fastpose_stream_from_state_dict(synth.synth_fastpose_state_dict(sk, args.nClasses), args.nClasses)
        else:
            ys = read_darknet_weights(args.yolo_weights or 'models/yolo/{:02d}.weights'.format(obj_id))[2]
            ks = fastpose_stream_from_state_dict(
                load_kpd_pkl(args.kpd_weights or './exp/final_model/' + ALLPATHS[obj_id] + '.pkl'), args.nClasses)
    ys, ks = bpd.broadcast_stream(ys), bpd.broadcast_stream(ks)
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=int(args.inp_dim), max_batch=max(1, args.detbatch), device=local)
    det.load_stream(ys).cuda()
    pose_model = FastPoseHIP.from_stream(ks, n_classes=args.nClasses, max_batch=max(1, args.detbatch, C_) if args.fused else 1,
                                        device=local).cuda()
    det.set_precision(args.precision)
    pose_model.set_precision(args.precision)

    t0 = time.time()
    if args.fused:
        from betapose_amd.frame_loader import FrameLoader
        from betapose_amd.pipeline import (POSE_DOUBLES, StreamedRunner, candidate_row_floats, finish_candidate_pose_record,
                                           finish_candidate_records, finish_pose_record, finish_record, unpack_candidate_row)
        mine = bpd.shard_indices(len(im_names), rank, world)
        # --candidates: a frame's record is its packed candidate row (C records, count and, with --device_pnp, the tail's outputs)
        # (and, with --all_instances on top, the instance pose rows)
        inst_dev = bool(C_ and args.device_pnp and args.all_instances)
        recs = np.zeros((len(mine), candidate_row_floats(C_, args.device_pnp, inst_dev) if C_ else 316), np.float32)
        poses = np.zeros((len(mine), POSE_DOUBLES), np.float64) if args.device_pnp and not C_ else None

        def keep(j, rec, pose=None):
            recs[j] = rec
            if pose is not None:
                poses[j] = pose
        t_dev = time.time()
        if len(mine):   # a rank beyond the frame count has nothing to load (its share of the gather is empty)
            # decode threads are a per-GPU budget: ranks of one node share the host cores
            threads = max(1, min(args.load_threads, (os.cpu_count() or 8) // max(1, world)))
            loader = FrameLoader([os.path.join(args.inputpath, im_names[i]) for i in mine], threads=threads,
                                 depth=max(16, 2 * args.streams * max(1, args.detbatch) + threads))
            runner = StreamedRunner(det, pose_model, loader.height, loader.width, streams=args.streams,
                                    confidence=args.confidence, num_classes=args.num_classes, batch=args.detbatch,
                                    pose_solver=(kp3d, cam_K, left_number, ransac) if args.device_pnp else None,
                                    candidates=C_ or None, nms_conf=args.nms_thesh, all_instances=inst_dev)
            runner.run(loader, keep)
            loader.close()
        t_dev = time.time() - t_dev
        print("rank %d: %d frames, files -> records %.1f frames/sec (%d launches of %d frame(s) in flight, %d decode threads)" % (
            rank, len(mine), len(mine) / max(t_dev, 1e-9), args.streams, max(1, args.detbatch), args.load_threads))
        allrec = bpd.gather_records(recs, mine, len(im_names))
        # the pose rows travel through the same gather, each f64 as a pair of f32 bit patterns
        allpose = bpd.gather_records(poses.view(np.float32), mine, len(im_names)) if poses is not None else None
        final_result = []
        if rank == 0:
            for i, name in enumerate(im_names):
                if C_:
                    rows, n, prow, merged, info = unpack_candidate_row(allrec[i], C_, args.device_pnp)
                    if inst_dev:
                        inst = unpack_candidate_row(allrec[i], C_, True, instances=True)[5]
                        out = finish_candidate_pose_record(rows, n, prow, merged, info, name, inst_poses=inst)
                    elif args.device_pnp:
                        out = finish_candidate_pose_record(rows, n, prow, merged, info, name)
                    else:
                        out = finish_candidate_records(rows, n, name, kp3d, cam_K, left_number, all_instances=args.all_instances)
                elif allpose is not None:
                    out = finish_pose_record(allrec[i], np.ascontiguousarray(allpose[i]).view(np.float64), name)
                else:
                    out = finish_record(allrec[i], name, kp3d, cam_K, left_number, ransac=ransac)
                if out["boxes"] is not None:
                    final_result.append(out)
    else:
        assert world == 1, "the staged pipeline is single-GPU; use --fused to shard frames over ranks"
        assert not args.device_pnp, "--device_pnp needs --fused (the device pose tail ends the fused frame graph)"
        from betapose_amd.dataloader import DataWriter, DetectionLoader, DetectionProcessor, ImageLoader
        data_loader = ImageLoader(im_names, batchSize=args.detbatch, format='yolo', reso=int(args.inp_dim)).start()
        det_loader = DetectionLoader(data_loader, obj_id, batchSize=args.detbatch, det_model=det).start()
        det_processor = DetectionProcessor(det_loader).start()
        writer = DataWriter(cam_K, left_number, kp3d, ransac=ransac).start()
        prof = {'dt': [], 'pt': [], 'pn': []}
        for i in range(data_loader.length()):
            t_s = time.time()
            (inps, orig_img, im_name, boxes, scores, pt1, pt2) = det_processor.read()
            if boxes is None or boxes.nelement() == 0:
                writer.save(None, None, None, None, None, orig_img, im_name.split('/')[-1])
                continue
            t_d = time.time()
            hm = pose_model(inps.cuda()).cpu()
            t_p = time.time()
            writer.save(boxes, scores, hm, pt1, pt2, orig_img, im_name.split('/')[-1])
            prof['dt'].append(t_d - t_s); prof['pt'].append(t_p - t_d); prof['pn'].append(time.time() - t_p)
        while writer.running():
            pass
        writer.stop()
        final_result = writer.results()
        if args.profile:
            print('det time: {:.4f} | pose time: {:.4f} | post processing: {:.5f}'.format(
                np.mean(prof['dt']), np.mean(prof['pt']), np.mean(prof['pn'])))
    if rank == 0:
        print('===========================> Finish Model Running: %d frames, %d with a pose, %.2f s' % (
            len(im_names), sum(len(f['result']) > 0 for f in final_result), time.time() - t0))
        if args.verify:     # before the JSON, the refinement and every error: they see the verified frame pose
            verify_frame_poses(args, obj_id, final_result, gt_frames, kp3d, cam_K, torch.device("cuda", local))
        write_json(final_result, args.outputpath)
        match = args.all_instances and not args.verify      # --verify: no ground-truth box takes part in the choice
        if gt_frames is not None:
            sym = obj_id in id_list(args.symmetric_ids)
            depth_inputs, m_ref = None, None
            if args.vsd or args.refine_depth is not None:
                depth_inputs = load_depth_inputs(args.sixd_base, obj_id, 2 if args.occlusion else None, final_result,
                                                 gt_frames, metric_cam)
            if args.refine_depth is not None:   # before any error: the lines below are those of the refined poses
                m_ref = refine_scored_poses(obj_id, final_result, gt_frames, model_vertices, depth_inputs, diameter,
                                            torch.device("cuda", local), args.refine_depth,
                                            match_instances=match)
            m = metrics.evaluate_results(final_result, gt_frames, model_vertices, metric_cam, diameter, pixel_thresh,
                                         symmetric=sym, device=torch.device("cuda", local) if sym else None,
                                         match_instances=match)
            print("Mean add accuracy for seq %02d is: %.3f" % (obj_id, m["mean_add"]))
            if sym:
                print("Mean add-s accuracy for seq %02d is: %.3f" % (obj_id, m["mean_adds"]))
            print("2d reprojection accuracy for seq %02d is: %.3f" % (obj_id, m["mean_2d_acc"]))
            print("Mean IoU for seq %02d is: %.3f" % (obj_id, m["mean_iou"]))
            if args.bop_metrics:
                print_bop_metrics(args.sixd_base, obj_id, final_result, gt_frames, model_vertices, metric_cam, diameter,
                                  torch.device("cuda", local), match_instances=match)
            if args.vsd and m_ref is not None:      # the refinement pass has scored the refined poses already
                print("Mean vsd recall for seq %02d is: %.3f" % (obj_id, m_ref["ar_vsd"]))
            elif args.vsd:
                print_vsd_metrics(args.sixd_base, obj_id, 2 if args.occlusion else None, final_result, gt_frames,
                                  model_vertices, metric_cam, diameter, torch.device("cuda", local),
                                  match_instances=match, depth_inputs=depth_inputs)
        elif (args.vsd or args.refine_depth is not None) and args.synthetic:
            print_synthetic_vsd(obj_id, final_result, kp3d, cam_K, synth_size, torch.device("cuda", local), vsd=args.vsd,
                                refine_iterations=args.refine_depth)
        if args.save_img:   # after the refinement: cam_R / cam_t hold the poses the lines above were scored on
            save_images(args, obj_id, final_result, gt_frames, kp3d, cam_K, torch.device("cuda", local))
    bpd.finalize()


if __name__ == "__main__":
    main()
