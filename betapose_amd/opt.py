"""Flags of the hot path -- same names and defaults as the reference's argparse singleton
(3_6Dpose_estimator/opt.py:1-150): the flags the inference path reads, plus the remaining ones accepted and ignored.  ``opt`` is a module-level
namespace like the reference's; ``parse_args`` refreshes it from a command line."""
from __future__ import annotations

import argparse


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Betapose per-frame inference on MI355X")
    p.add_argument('--left_keypoints', default=10, type=int, help='key points kept for PnP on Occlusion-LineMod')
    p.add_argument('--obj_id', default=5, type=int)
    p.add_argument('--sp', default=False, action='store_true', help='single process (threads); the only mode here')
    p.add_argument('--profile', default=False, action='store_true')
    p.add_argument('--nClasses', default=50, type=int)
    p.add_argument('--fast_inference', default=True, type=bool)
    p.add_argument('--inputResH', default=320, type=int)
    p.add_argument('--inputResW', default=256, type=int)
    p.add_argument('--outputResH', default=80, type=int)
    p.add_argument('--outputResW', default=64, type=int)
    p.add_argument('--indir', dest='inputpath', default='')
    p.add_argument('--list', dest='inputlist', default='')
    p.add_argument('--mode', dest='mode', default='normal')
    p.add_argument('--outdir', dest='outputpath', default='examples/res/')
    p.add_argument('--inp_dim', dest='inp_dim', type=str, default='416')
    p.add_argument('--conf', dest='confidence', type=float, default=0.01)
    p.add_argument('--nms', dest='nms_thesh', type=float, default=0.6)
    p.add_argument('--save_img', default=False, action='store_true',
                   help='write <outdir>/vis/<imgname>.png: the frame with the estimated pose(s) drawn as shaded mesh and '
                        '3-D box, the ground-truth box in green')
    p.add_argument('--vis', default=False, action='store_true',
                   help='accepted for the reference command lines and unused: there is no display, use --save_img')
    p.add_argument('--format', type=str, default=None)
    p.add_argument('--detbatch', type=int, default=1)
    p.add_argument('--posebatch', type=int, default=80)
    p.add_argument('--save_video', dest='save_video', default=False, action='store_true')
    # additions of this implementation
    p.add_argument('--occlusion', default=False, action='store_true',
                   help='Occlusion-LineMod protocol (occlusion_betapose_evaluate.py): GT sequence 02, every GT object of a '
                        'frame, --left_keypoints for PnP, 20 px reprojection threshold')
    p.add_argument('--obj_ids', default='', type=str,
                   help='occlusion_evaluate.py: comma-separated object ids evaluated in ONE run, e.g. 1,5,6,8,9,10,11,12 -- '
                        'units of work are (frame, object) pairs, every object keeps its weights resident, frames are '
                        'decoded once')
    p.add_argument('--symmetric_ids', default='', type=str,
                   help='comma-separated object ids scored with ADD-S as well (LineMod\'s symmetric objects are 10, eggbox, '
                        'and 11, glue): one more line per such object, "Mean add-s accuracy for seq XX is: ...", computed '
                        'on the run\'s GPU (metrics.pose_errors)')
    p.add_argument('--bop_metrics', default=False, action='store_true',
                   help='also score every evaluated object with the BOP symmetry-aware errors MSSD and MSPD, over the '
                        'symmetry set its models_info.yml entry declares (symmetries_discrete / symmetries_continuous; '
                        'none: the identity), as average recall over the ten BOP thresholds: two more lines per object, '
                        '"Mean mssd recall for seq XX is: ..." and "Mean mspd recall for seq XX is: ...", computed on the '
                        'run\'s GPU (metrics.pose_errors_sym)')
    p.add_argument('--vsd', default=False, action='store_true',
                   help='also score every evaluated object with BOP\'s Visible Surface Discrepancy: reads the faces of '
                        'models/obj_XX.ply and the 16-bit depth images <sequence>/depth/NNNN.png, renders the ground-truth '
                        'and the estimated pose of every scored pair on the run\'s GPU (metrics.pose_errors_vsd) and prints '
                        'one more line per object, "Mean vsd recall for seq XX is: ...", the average recall over the BOP '
                        'taus and thresholds.  With --synthetic the run scores its own poses against depth images rendered '
                        'from them (a closed loop that only exercises the path)')
    p.add_argument('--refine_depth', nargs='?', type=int, default=None, const=8, metavar='ITERS',
                   help='refine every scored pose against its frame\'s depth image before any error is computed: projective '
                        'point-to-plane ICP on the run\'s GPU (metrics.refine_poses_depth; ITERS iterations, default 8).  Reads '
                        'the mesh faces and the depth PNGs --vsd reads; the accuracy lines are then those of the refined '
                        'poses, and one more line per object gives the numbers refined / rejected / unchanged and the mean rms '
                        'residual before and after.  With --synthetic the run refines its own poses against depth images '
                        'rendered from them (a closed loop that only exercises the path).  Default: off')
    p.add_argument('--shared_detector', default='', type=str, metavar='CFG[,WEIGHTS]',
                   help='occlusion_evaluate.py --obj_ids: ONE multi-class detector (Darknet cfg, .weights file) serves every '
                        'object -- one resize and one detector pass per frame, the best box of each object\'s class, then each '
                        'object\'s key-point chain in the same graph (DESIGN.md 3.6).  With --synth_weights the weights are '
                        'seeded synthetic ones and only CFG is read.  Frames, not units, are sharded over the ranks')
    p.add_argument('--class_map', default='', type=str, metavar='OBJ:CLASS,...',
                   help='--shared_detector: detector class of each object id, e.g. 1:0,5:1,6:2; default: the position of the '
                        'id in LineMod\'s sorted id list 1..15 (class = id - 1, as the reference\'s 15-class labels are written)')
    p.add_argument('--candidates', type=int, default=0, metavar='C',
                   help='--fused: up to C (1..8) box-NMS survivors per frame (--nms is the IoU threshold) go through one '
                        'key-point pass at batch C and are merged by pPose-NMS; PnP on result[0] (DESIGN.md 3.7).  Alone '
                        'or with --device_pnp; not with --pnp_ransac or --shared_detector')
    p.add_argument('--all_instances', default=False, action='store_true',
                   help='--candidates C: a pose for EVERY merged pose pPose-NMS leaves, not result[0] alone -- each JSON entry '
                        'carries its own cam_R / cam_t and the scoring matches ground-truth entries to instances by box IoU '
                        '(DESIGN.md 3.7).  Alone or with --device_pnp (one more launch at the end of the frame graph)')
    p.add_argument('--verify', nargs='?', default=None, const='device', choices=['device', 'host'],
                   help='--candidates C --all_instances: choose the frame\'s pose among its instance poses by looking at the '
                        'image -- every solved instance is rendered with the object\'s coloured mesh and scored by the agreement '
                        'of its unit Sobel gradients with the frame\'s (the reference\'s verify_6D_poses; DESIGN.md 3.18), on the '
                        'run\'s GPU (or with "host" by the byte-identical host twin).  The best becomes cam_R / cam_t before '
                        '--refine_depth and before scoring, which then takes the frame pose as it is (no ground-truth box '
                        'picks an instance); one more line gives the frames scored and the choices changed.  Default: off')
    p.add_argument('--fused', default=False, action='store_true', help='one hipGraph per frame instead of stage threads')
    p.add_argument('--device_pnp', default=False, action='store_true',
                   help='--fused: key-point decode, pPose-NMS, pruning and PnP on each rank\'s GPU at the end of the frame '
                        'graph (the device pose tail, DESIGN.md 3.5); rank 0 only builds the result dicts')
    p.add_argument('--pnp_ransac', nargs='?', type=float, default=None, const=12.0, metavar='PX',
                   help='solve the pose with the RANSAC variant the reference keeps commented out (utils/utils.py:32-36): '
                        'reprojection error in pixels (default 12.0), 100 trials, confidence 0.99; in the host tail and, '
                        'with --device_pnp, on the GPU with the hypotheses in parallel (DESIGN.md 3.5)')
    p.add_argument('--synthetic', type=int, default=0, help='run on N seeded synthetic frames / weights')
    p.add_argument('--synth_weights', default=False, action='store_true',
                   help='seeded synthetic weights with real frames / ground truth (plumbing runs without checkpoints)')
    p.add_argument('--precision', choices=['f32', 'bf16x3', 'f16'], default='bf16x3',
                   help='matrix-core operand precision: bf16x3 (default: fp32-accurate 3-way bf16 split), f32 (fp32 MFMA), f16 (fp16 operands, '
                        'fp32 accumulate); see DESIGN.md 3.1b/c')
    p.add_argument('--streams', type=int, default=4, help='--fused: frames in flight (HIP streams / engine clones)')
    p.add_argument('--load_threads', type=int, default=8, help='--fused: PNG decode threads')
    p.add_argument('--sixd_base', default='/media/data_2/SIXD/hinterstoisser')
    p.add_argument('--yolo_weights', default='')
    p.add_argument('--kpd_weights', default='')
    # the rest of the reference's flag set (training, visualisation, video input: opt.py:9-150) -- accepted with the
    # reference's names, types and defaults so that existing command lines and scripts keep parsing; nothing on the
    # inference path reads them
    for name, default, typ in _COMPAT_FLAGS:
        kw = {"default": default, "help": argparse.SUPPRESS}
        if typ is not None:
            kw["type"] = typ
        p.add_argument(name, **kw)
    p.add_argument('--dist', dest='dist', type=int, default=1, help=argparse.SUPPRESS)
    p.add_argument('--backend', dest='backend', type=str, default='gloo', help=argparse.SUPPRESS)
    p.add_argument('--port', dest='port', default=None, help=argparse.SUPPRESS)
    p.add_argument('--net', dest='demo_net', default='res152', help=argparse.SUPPRESS)
    p.add_argument('--video', dest='video', default="", help=argparse.SUPPRESS)
    p.add_argument('--webcam', dest='webcam', type=str, default='0', help=argparse.SUPPRESS)
    p.add_argument('--vis_fast', dest='vis_fast', default=False, action='store_true', help=argparse.SUPPRESS)
    return p


_COMPAT_FLAGS = [
    ('--expID', 'default', str), ('--dataset', 'coco', str), ('--nThreads', 40, int), ('--debug', False, bool),
    ('--snapshot', 1, int), ('--addDPG', False, bool), ('--netType', 'hgPRM', str), ('--loadModel', None, str),
    ('--Continue', False, bool), ('--nFeats', 256, int), ('--nStack', 4, int), ('--use_pyranet', True, bool),
    ('--LR', 2.5e-4, float), ('--momentum', 0, float), ('--weightDecay', 0, float), ('--crit', 'MSE', str),
    ('--optMethod', 'rmsprop', str), ('--nEpochs', 200, int), ('--epoch', 0, int), ('--trainBatch', 40, int),
    ('--validBatch', 20, int), ('--trainIters', 0, int), ('--valIters', 0, int), ('--init', None, str),
    ('--scale', 0.25, float), ('--rotate', 30, float), ('--hmGauss', 1, int), ('--baseWidth', 9, int),
    ('--cardinality', 5, int), ('--nResidual', 1, int),
]


opt = build_parser().parse_args([])
opt.num_classes = 80            # opt.py:150


def id_list(text: str):
    """'10, 11' -> [10, 11] (--obj_ids, --symmetric_ids)."""
    return [int(v) for v in text.split(",") if v.strip()]


LINEMOD_IDS = list(range(1, 16))     # the 15 LineMod objects; the reference's multi-object labels use obj_id - 1


def shared_detector_arg(text: str):
    """'CFG' or 'CFG,WEIGHTS' (--shared_detector) -> (cfg path, weights path or None)."""
    parts = [v.strip() for v in text.split(",")]
    if not 1 <= len(parts) <= 2 or not all(parts):
        raise ValueError("--shared_detector takes CFG or CFG,WEIGHTS, not %r" % text)
    return parts[0], (parts[1] if len(parts) == 2 else None)


def class_map(text: str, obj_ids):
    """--class_map 'OBJ:CLASS,...' -> {obj_id: class id} for ``obj_ids``.  Empty text: the position of each id in the
    sorted LineMod id list.  Every object needs a class, and no two objects may share one."""
    if text.strip():
        m = {}
        for item in text.split(","):
            if not item.strip():
                continue
            try:
                o, c = item.split(":")
                o, c = int(o), int(c)
            except ValueError:
                raise ValueError("--class_map: %r is not OBJ:CLASS" % item.strip())
            if o in m:
                raise ValueError("--class_map: object %d listed twice" % o)
            m[o] = c
    else:
        m = {o: LINEMOD_IDS.index(o) for o in obj_ids if o in LINEMOD_IDS}
    missing = [o for o in obj_ids if o not in m]
    if missing:
        raise ValueError("--class_map: no detector class for objects %s" % missing)
    out = {o: m[o] for o in obj_ids}
    if len(set(out.values())) != len(out):
        raise ValueError("--class_map: two objects share a detector class in %s" % out)
    if min(out.values()) < 0:
        raise ValueError("--class_map: negative class id in %s" % out)
    return out


def parse_args(argv=None):
    global opt
    ns = build_parser().parse_args(argv)
    ns.num_classes = 80
    opt.__dict__.update(ns.__dict__)
    return opt
