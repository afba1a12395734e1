"""Shared multi-class detector: one YOLO pass per frame, the per-class select kernel
(csrc/yolo_tail.hip yolo_select_classes_kernel, from the prediction tensor and from the head tensors), and ``ScenePipeline`` -- every
object's crop -> key-point net -> arg-max -> pose tail behind that one pass, in one graph.

Inputs: ``helpers.frames``, the 15-class YOLOv3 cfg at 416 with ``synth_yolo_stream(1, blocks)``.  Checked once on the CPU
with ``oracle.yolo_ref`` on frames 0..2: at confidence 0.01 every one of the 15 classes has a candidate row (the rarest,
class 5, has one or two), at 0.6 classes 0, 1, 4, 5, 7 and 8 have none while 2, 6, 9, 10, 11, 12 and 14 keep tens to
thousands.

Bars: everything here is bit-identity -- the select against a float32 numpy restatement of its rule on the same
prediction tensor, the two forms of the kernel against each other, the class list [0] against today's select, a scene
row against today's ``FramePipeline`` on a detector whose head filters have that class and class 0 swapped (the same
convolution arithmetic in another output column), graph replay against the eager launches."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers  # noqa: E402
from betapose_amd import cfg as C, synth, weights as W  # noqa: E402
from betapose_amd.darknet import Darknet  # noqa: E402
from betapose_amd.kpd import FastPoseHIP  # noqa: E402
from betapose_amd.pipeline import (POSE_DOUBLES, RESULT_FLOATS, FramePipeline, MultiObjectRunner, ScenePipeline,  # noqa: E402
                                   finish_pose_record, frame_sharded_owner)
from betapose_amd.weights import fastpose_stream_from_state_dict  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CLASSES = 15
CONF, CONF_SPARSE = 0.01, 0.6
OBJS = [1, 5, 6, 8]                                  # LineMod ids; detector class = id - 1 (the default map)
CLASS_OF = {o: o - 1 for o in OBJS}
LEFT = 10


def _blocks15():
    return C.parse_cfg_text(C.yolov3_single_cfg_text(classes=N_CLASSES))


def _det15(stream=None, precision=None):
    d = Darknet("yolo/cfg/yolov3-single.cfg", reso=416)
    d.blocks = _blocks15()
    d.net_info = d.blocks[0]
    d.load_stream(synth.synth_yolo_stream(helpers.YOLO_SEED, _blocks15()) if stream is None else stream).cuda()
    if precision:
        d.set_precision(precision)
    return d


def _pose(obj, precision=None):
    sk = synth.object_seeds(obj)[1]
    p = FastPoseHIP.from_stream(fastpose_stream_from_state_dict(synth.synth_fastpose_state_dict(sk, 50), 50), n_classes=50).cuda()
    if precision:
        p.set_precision(precision)
    return p


def _kp3d(obj):
    return synth.synth_kp3d(50, seed=7 + obj)


def _swapped_stream(c):
    """The 15-class stream with the filters and biases of class ``c`` and class 0 swapped, per anchor, in the three head
    convolutions: the detector's class-0 output column then carries what class ``c``'s carried."""
    blocks = _blocks15()
    flat = synth.synth_yolo_stream(helpers.YOLO_SEED, blocks).copy()
    heads = [e for e in W.darknet_stream_layout(blocks) if not e["bn"]]
    assert len(heads) == 3
    attrs = 5 + N_CLASSES
    for e in heads:
        co, fan = e["cout"], e["cin"] * e["k"] ** 2
        assert co == 3 * attrs
        bias = flat[e["bias"]:e["bias"] + co]
        w = flat[e["weight"]:e["weight"] + co * fan].reshape(co, fan)
        for a in range(3):
            i, j = a * attrs + 5, a * attrs + 5 + c
            bias[[i, j]] = bias[[j, i]]
            w[[i, j]] = w[[j, i]]
    return flat


@pytest.fixture(scope="module")
def det15(cuda):
    return _det15()


@pytest.fixture(scope="module")
def poses(cuda):
    return {o: _pose(o) for o in OBJS}


@pytest.fixture(scope="module")
def xs(cuda):
    return torch.cat([helpers.yolo_input_from_frame(f) for f in helpers.frames(3)]).cuda()


def _scene(det, poses, objs=OBJS, solver=True, use_graph=True, frames=None):
    sp = ScenePipeline(det, {o: poses[o] for o in objs}, CLASS_OF, 480, 640, confidence=CONF, use_graph=use_graph, frames=frames)
    if solver:
        for o in objs:
            sp.set_pose_solver(o, _kp3d(o), synth.CAM_K, LEFT)
    return sp


def _run_scene(sp, frame):
    rows = sp.run(frame).copy()
    pose_rows = sp.poses.cpu().numpy().copy() if sp.poses is not None else None
    return rows, pose_rows


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _select_ref(pred, conf, num_classes, class_ids):
    """The rule of the kernel restated in float32 numpy on one image's [rows][attrs] tensor: objectness > conf, arg-max
    class (first maximum) over min(num_classes, attrs - 5) scores, per listed class the highest objectness (lowest row
    on ties); record = (row as int bits, x1, y1, x2, y2, objectness, class score, class id), -1 and zeros when empty."""
    pred = np.asarray(pred, dtype=np.float32)
    ncls = min(num_classes, pred.shape[1] - 5)
    obj = pred[:, 4]
    cls = np.argmax(pred[:, 5:5 + ncls], axis=1)           # first maximum
    out = np.zeros((len(class_ids), 8), np.float32)
    idx = np.full(len(class_ids), -1, np.int32)
    for k, c in enumerate(class_ids):
        cand = np.nonzero((obj > np.float32(conf)) & (cls == c))[0]
        if len(cand):
            r = int(cand[np.argmax(obj[cand])])             # first maximum among ascending rows
            idx[k] = r
            q = pred[r]
            two = np.float32(2)
            out[k, 1] = q[0] - q[2] / two
            out[k, 2] = q[1] - q[3] / two
            out[k, 3] = q[0] + q[2] / two
            out[k, 4] = q[1] + q[3] / two
            out[k, 5] = q[4]
            out[k, 6] = q[5 + c]
            out[k, 7] = np.float32(c)
    out[:, 0] = idx.view(np.float32)
    return out, idx


def test_plain_select_on_seeded_tensors_is_the_restatement_bit_for_bit(cuda):
    """The tensor form of the single select (``ops.select``: the one-slot instantiation of the per-class select with the
    list [0]) against ``_select_ref(pred, conf, num_classes, [0])``, all eight floats of every image equal as bytes.
    rows 17 / 1025 / 2535: under one sweep of the block's 1 024 threads, one row past it, several sweeps;
    (attrs, num_classes) so that min(num_classes, attrs - 5) is 1, 2 (num_classes binds), 80 (attrs binds), 2 of 80 scores.
    Per trial of three images: [0] nothing above the threshold (one row AT it), [1] an exact three-way tie on the best
    objectness, the last row among them (the first must win; one of the three also ties its class scores, first maximum
    = class 0), [2] the top-objectness row has first-max class 1 and the runner-up, of class 0, must win."""
    from betapose_amd import ops
    rng = np.random.default_rng(11)
    f32 = np.float32
    seen_empty = seen_full = seen_tie = seen_other = 0
    for trial, (rows, (attrs, nc)) in enumerate((r, an) for r in (17, 1025, 2535) for an in ((6, 80), (8, 2), (85, 80), (85, 2))):
        ncls = min(nc, attrs - 5)
        conf = (0.01, 0.5, 0.9)[trial % 3]
        pred = np.zeros((3, rows, attrs), f32)
        pred[..., 0:2] = rng.uniform(0, 416, (3, rows, 2))
        pred[..., 2:4] = rng.uniform(2, 300, (3, rows, 2))
        pred[..., 4] = rng.uniform(0, 1, (3, rows)) ** 3 * 0.97
        pred[..., 5:] = rng.uniform(0, 0.9, (3, rows, attrs - 5))
        pred[0, :, 4] *= f32(conf * 0.5)
        pred[0, rows // 2, 4] = f32(conf)                        # objectness == conf is not above it
        tie = np.sort(np.append(rng.choice(rows - 1, 2, replace=False), rows - 1))
        pred[1, tie, 4] = f32(0.995)
        pred[1, tie, 5] = f32(0.95)                              # class 0 is their arg-max ...
        if ncls > 1:
            pred[1, tie[0], 6] = f32(0.95)                       # ... also where class 1 scores the same
        top, second = rng.choice(rows, 2, replace=False)
        pred[2, top, 4], pred[2, second, 4] = f32(0.99), f32(0.98)
        pred[2, second, 5] = f32(0.95)
        if ncls > 1:
            pred[2, top, 6] = f32(0.95)
        ref = np.stack([_select_ref(pred[b], conf, nc, [0])[0][0] for b in range(3)])
        idx = ref[:, 0].copy().view(np.int32)
        print("trial %d rows %d attrs %d num_classes %d conf %.2f -> rows %s" % (trial, rows, attrs, nc, conf, idx.tolist()))
        assert idx[0] == -1 and (pred[0, :, 4] == f32(conf)).any()
        assert (pred[1, :, 4] == pred[1, :, 4].max()).sum() == 3 and idx[1] == tie[0] < tie[1] < tie[2]
        assert idx[2] == (second if ncls > 1 else top) and int(np.argmax(pred[2, :, 4])) == top
        seen_empty += int((idx < 0).sum())
        seen_full += int((idx >= 0).sum())
        seen_tie += 1
        seen_other += int(ncls > 1)
        got = ops.select(torch.from_numpy(pred).to(cuda), confidence=conf, num_classes=nc).cpu().numpy()
        assert got.shape == (3, 8)
        np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg="trial %d" % trial)
    assert seen_empty > 0 and seen_full > 0 and seen_tie == 12 and seen_other > 0, "input conditions"


@pytest.mark.parametrize("class_ids", [list(range(N_CLASSES)), [7, 0, 12]])
def test_select_against_numpy_restatement(det15, xs, class_ids):
    seen_empty = seen_full = 0
    for conf in (CONF, CONF_SPARSE):
        for n in range(3):
            _, pred = det15.forward_select(xs[n:n + 1], confidence=conf, want_pred=True)
            sel, pred2 = det15.forward_select_classes(xs[n:n + 1], class_ids, confidence=conf, want_pred=True)
            assert tuple(sel.shape) == (1, len(class_ids), 8) and torch.equal(pred, pred2)
            got = sel.cpu().numpy()[0]
            ref, idx = _select_ref(pred.cpu().numpy()[0], conf, 80, class_ids)
            print("conf %.2f frame %d classes %s rows %s" % (conf, n, class_ids, idx.tolist()))
            np.testing.assert_array_equal(got[:, :1].copy().view(np.int32)[:, 0], idx)
            np.testing.assert_array_equal(_bits(got), _bits(ref))
            if conf == CONF:
                assert (idx >= 0).all(), "input condition: every class has a candidate at confidence 0.01"
            else:
                seen_empty += int((idx < 0).sum())
                seen_full += int((idx >= 0).sum())
                empty = got[idx < 0]
                assert (empty[:, 1:] == 0).all() and (empty[:, :1].copy().view(np.int32) == -1).all()
    assert seen_empty > 0 and seen_full > 0, "input condition: confidence 0.6 empties some classes, not all"


def test_both_forms_agree(det15, xs):
    for ids, conf in ((list(range(N_CLASSES)), CONF), (list(range(N_CLASSES)), CONF_SPARSE), ([7, 0, 12], CONF)):
        for n in range(3):
            a = det15.forward_select_classes(xs[n:n + 1], ids, confidence=conf)
            b, _ = det15.forward_select_classes(xs[n:n + 1], ids, confidence=conf, want_pred=True)
            np.testing.assert_array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


def test_class_list_zero_is_todays_select(cuda, xs):
    det1 = Darknet("yolo/cfg/yolov3-single.cfg", reso=416).load_stream(helpers.yolo_stream()).cuda()
    for conf in (CONF, 0.999):
        for want_pred in (False, True):
            for n in range(3):
                old = det1.forward_select(xs[n:n + 1], confidence=conf, want_pred=want_pred)
                new = det1.forward_select_classes(xs[n:n + 1], [0], confidence=conf, want_pred=want_pred)
                old, new = (old[0], new[0]) if want_pred else (old, new)
                np.testing.assert_array_equal(_bits(old.cpu().numpy()), _bits(new.cpu().numpy()[:, 0]))
    with pytest.raises(ValueError):
        det1.forward_select_classes(xs[:1], [1])             # a single-class cfg has class 0 only


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_scene_row_is_todays_pipeline_on_the_permuted_detector(cuda, precision):
    """For class c != 0 the detector with class c's and class 0's head filters swapped reports, as ITS class 0, what the
    shared detector reports as class c; today's FramePipeline on it (pose tail on) must write the scene's row for c:
    all 316 floats and the 166 pose doubles bit-identical, select slots [6] and [7] aside."""
    objs = [1, 5, 8]                                         # classes 0, 4, 7: two swapped classes are checked
    det = _det15(precision=precision)
    pose = {o: _pose(o, precision) for o in objs}
    sp = _scene(det, pose, objs)
    frames = helpers.frames(3)
    scene_rows = [_run_scene(sp, f) for f in frames]
    for o in objs[1:]:
        c = CLASS_OF[o]
        det_c = _det15(_swapped_stream(c), precision)
        fp = FramePipeline(det_c, pose[o], 480, 640, batch=1, confidence=CONF)
        fp.set_pose_solver(_kp3d(o), synth.CAM_K, LEFT)
        k = objs.index(o)
        for f, (rows, pose_rows) in zip(frames, scene_rows):
            rec = fp.run(f)[0].copy()
            prow = fp.poses.cpu().numpy()[0].copy()
            i_s, i_p = rows[k, :1].copy().view(np.int32)[0], rec[:1].view(np.int32)[0]
            print("precision %s class %d: scene row %d, pipeline row %d" % (precision, c, i_s, i_p))
            assert i_s == i_p and i_s >= 0
            assert rows[k, 7] == float(c) and rec[7] == 0.0
            keep = np.ones(RESULT_FLOATS, bool)
            keep[6:8] = False
            np.testing.assert_array_equal(_bits(rows[k][keep]), _bits(rec[keep]))
            np.testing.assert_array_equal(_bits(pose_rows[k]), _bits(prow))
        del fp, det_c


def test_graph_replay_and_kernel_counts(det15, poses):
    frames = helpers.frames(3)
    eager = _scene(det15, poses, use_graph=False)
    graph = _scene(det15, poses, use_graph=True).prepare()
    e0 = _run_scene(eager, frames[0])
    g0 = _run_scene(graph, frames[0])
    for a, b in zip(e0, g0):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    g1 = _run_scene(graph, frames[1])                         # replay on a second frame == a fresh scene on that frame
    del eager, graph
    fresh = _run_scene(_scene(det15, poses), frames[1])
    for a, b in zip(g1, fresh):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert not np.array_equal(g0[0], g1[0])

    # launches per frame.  A K = 1 scene makes the single pipeline's launches (another select kernel, the same number);
    # every further object adds its chain = crop + key-point net + arg-max + pose tail, i.e. the single count minus the
    # part in front of the crop (resize + detector + select).  That part is taken from the counts themselves:
    # front = single - (scene_2 - scene_1).
    fp = FramePipeline(det15, poses[OBJS[0]], 480, 640, batch=1, confidence=CONF)
    fp.set_pose_solver(_kp3d(OBJS[0]), synth.CAM_K, LEFT)
    single = fp.prepare().kernel_count()
    counts = {k: _scene(det15, poses, OBJS[:k]).prepare().kernel_count() for k in (1, 2, 4)}
    print("graph nodes: single pipeline %d, scenes %s" % (single, counts))
    assert counts[1] == single
    chain = counts[2] - counts[1]
    front = single - chain
    assert 0 < chain < single and front > 0
    assert counts[4] == single + 3 * (single - front)
    assert counts[4] < 4 * single


@pytest.fixture(scope="module")
def own_poses(cuda):
    """Two key-point engines of this test's own (their precision is toggled): object 1 at max_batch 2, object 5."""
    def make(obj, max_batch):
        stream = fastpose_stream_from_state_dict(synth.synth_fastpose_state_dict(synth.object_seeds(obj)[1], 50), 50)
        return FastPoseHIP.from_stream(stream, n_classes=50, max_batch=max_batch).cuda().set_precision("bf16x3")
    return {1: make(1, 2), 5: make(5, 1)}


@pytest.mark.parametrize("chain", ["pipeline", "scene", "cands"])
def test_graph_follows_a_plan_change(det15, own_poses, chain):
    """The rule the three chains share (csrc/frame_chain.h): a captured graph is rebuilt when an engine's launch plan
    changed or the pose tail was toggled.  After ``set_precision`` on ONE key-point engine the graph chain must write what
    a fresh eager chain over the same engines writes, bit for bit; the pose tail is one graph node."""
    from betapose_amd.pipeline import CandidatePipeline
    objs = [1, 5]
    frame = helpers.frames(1)[0]
    if chain == "pipeline":
        changed = own_poses[1]

        def make(use_graph):
            return FramePipeline(det15, own_poses[1], 480, 640, batch=1, confidence=CONF, use_graph=use_graph)

        def solver(c, on):
            c.set_pose_solver(*((_kp3d(1), synth.CAM_K, LEFT) if on else ()))
    elif chain == "scene":
        changed = own_poses[5]                                # the second slot's engine

        def make(use_graph):
            return _scene(det15, own_poses, objs, solver=False, use_graph=use_graph)

        def solver(c, on):
            for o in objs if on else objs[1:]:               # off: the second slot's tail alone
                c.set_pose_solver(o, *((_kp3d(o), synth.CAM_K, LEFT) if on else ()))
    else:
        changed = own_poses[1]

        def make(use_graph):
            return CandidatePipeline(det15, own_poses[1], 480, 640, candidates=2, confidence=CONF, class_id=CLASS_OF[1],
                                     use_graph=use_graph)

        def solver(c, on):
            c.set_pose_solver(*((_kp3d(1), synth.CAM_K, LEFT) if on else ()))

    def run(c):
        c.run(frame)
        return _bits(c.results.cpu().numpy()).copy(), _bits(c.poses.cpu().numpy()).copy()

    g = make(True)
    solver(g, True)
    first = run(g)
    changed.set_precision("f32")
    try:
        at_f32 = run(g)
        ref = make(False)
        solver(ref, True)
        ref = run(ref)
    finally:
        changed.set_precision("bf16x3")
    assert not np.array_equal(at_f32[0], first[0]), "input condition: the precision moves the key-point record"
    for a, b in zip(at_f32, ref):
        np.testing.assert_array_equal(a, b)

    back = run(g)
    n_on = g.kernel_count()
    solver(g, False)
    g.run(frame)
    n_off = g.kernel_count()
    solver(g, True)
    again = run(g)
    print("%s: graph nodes with the tail %d, without %d" % (chain, n_on, n_off))
    assert n_off == n_on - 1 and g.kernel_count() == n_on
    for a, b, c in zip(first, back, again):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)


def _write_frames(tmp_path, frames):
    from PIL import Image
    indir = tmp_path / "rgb"
    indir.mkdir()
    for i, fr in enumerate(frames):
        Image.fromarray(fr[:, :, ::-1].copy()).save(indir / ("%04d.png" % i))
    return indir


def test_runner_delivers_the_scene_rows(det15, poses, tmp_path):
    from betapose_amd.frame_loader import FrameLoader
    frames = helpers.frames(4)
    indir = _write_frames(tmp_path, frames)
    lone = _scene(det15, poses)
    want = [_run_scene(lone, f) for f in frames]
    del lone
    K = len(OBJS)
    solvers = {o: (_kp3d(o), synth.CAM_K, LEFT) for o in OBJS}
    runner = MultiObjectRunner({o: poses[o] for o in OBJS}, OBJS, 480, 640, streams=2, confidence=CONF, pose_solvers=solvers,
                               shared_detector=(det15, CLASS_OF))
    for world, rank in ((1, 0), (2, 1)):
        owner = frame_sharded_owner(K, world)
        mine = [f for f in range(len(frames)) if owner(f * K) == rank]
        loader = FrameLoader([str(indir / ("%04d.png" % f)) for f in mine], threads=2, depth=8)
        got = {}
        n = runner.run(loader, mine, lambda u: owner(u) == rank, lambda u, rec, pose: got.__setitem__(u, (rec, pose)))
        loader.close()
        assert n == len(mine) * K and sorted(got) == [f * K + oi for f in mine for oi in range(K)]
        for u, (rec, pose) in got.items():
            np.testing.assert_array_equal(_bits(rec), _bits(want[u // K][0][u % K]))
            np.testing.assert_array_equal(_bits(pose), _bits(want[u // K][1][u % K]))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _harness(nproc, args, timeout=900):
    """One run of occlusion_evaluate.py under its own timeout; a failing exit status stops the test there."""
    env = dict(os.environ, BP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = os.path.join(ROOT, "occlusion_evaluate.py")
    if nproc == 1:
        cmd = [sys.executable, script] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
               "127.0.0.1", "--master-port", str(_port()), script] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_harness_shared_detector(det15, tmp_path):
    """occlusion_evaluate.py --obj_ids 1,5,6 --shared_detector CFG --synth_weights --device_pnp on synthetic frames and a
    synthetic SIXD tree: per-object JSON equal to what finish_pose_record makes of a lone ScenePipeline's rows, and
    byte-identical between 1 rank and 2 gloo ranks on the one GPU."""
    sys.path.insert(0, ROOT)
    import evaluate
    from betapose_amd.pPose_nms import write_json
    objs = [1, 5, 6]
    frames = helpers.frames(3)
    indir = _write_frames(tmp_path, frames)
    cfg_path = tmp_path / "yolo-15.cfg"
    cfg_path.write_text(C.yolov3_single_cfg_text(classes=N_CLASSES))
    kp_mm = {o: np.round(_kp3d(o) * 1000.0, 6) for o in objs}
    gt = {i: [(o, np.eye(3), np.array([0.0, 0.0, 800.0]), [5, 5, 20, 20]) for o in objs] for i in range(len(frames))}
    rng = np.random.default_rng(0)
    base = str(tmp_path / "sixd")
    synth.write_sixd_tree(base, 2, gt, {o: rng.normal(size=(300, 3)) * 30.0 for o in objs}, kp_mm, {o: 100.0 for o in objs})

    pose = {o: _pose(o) for o in objs}
    sp = ScenePipeline(det15, pose, {o: o - 1 for o in objs}, 480, 640, confidence=CONF)
    for o in objs:
        sp.set_pose_solver(o, evaluate.load_sixd_gt(base, o, 2)[2], synth.CAM_K, LEFT)
    rows = [_run_scene(sp, f) for f in frames]
    want = {}
    for k, o in enumerate(objs):
        res = [finish_pose_record(rows[f][0][k], rows[f][1][k], "%04d.png" % f) for f in range(len(frames))]
        res = [r for r in res if r["boxes"] is not None]
        assert len(res) == len(frames)
        odir = tmp_path / "want" / ("obj_%02d" % o)
        os.makedirs(odir)
        write_json(res, str(odir))
        want[o] = open(odir / "Betapose-results.json").read()
    del sp, pose

    common = ["--indir", str(indir), "--sixd_base", base, "--synth_weights", "--fused", "--device_pnp", "--left_keypoints",
              str(LEFT), "--streams", "2", "--obj_ids", "1,5,6", "--shared_detector", str(cfg_path)]
    for nproc in (1, 2):
        out = _harness(nproc, common + ["--outdir", str(tmp_path / ("m%d" % nproc))])
        assert "shared detector" in out
        for o in objs:
            got = open(tmp_path / ("m%d" % nproc) / ("obj_%02d" % o) / "Betapose-results.json").read()
            assert len(json.loads(got)) == len(frames)
            assert got == want[o], "object %d, %d rank(s)" % (o, nproc)
