"""Host side of the shared multi-class detector (no GPU): the harness options, frame-sharded unit ownership, the
exported ``bp_scene_*`` / ``bp_yolo_forward_select_classes`` entry points and the class-list checks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import helpers
from betapose_amd import _lib, cfg as Cfg
from betapose_amd.darknet import Darknet, check_class_ids
from betapose_amd.opt import LINEMOD_IDS, build_parser, class_map, id_list, shared_detector_arg
from betapose_amd.pipeline import ScenePipeline, frame_sharded_owner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bp_yolo_forward_select_classes", "bp_scene_create", "bp_scene_destroy", "bp_scene_results", "bp_scene_poses",
           "bp_scene_set_pose_solver", "bp_scene_set_pose_ransac", "bp_scene_prepare", "bp_scene_run", "bp_scene_kernel_count"]


def test_shared_detector_and_class_map_options():
    p = build_parser()
    ns = p.parse_args([])
    assert ns.shared_detector == "" and ns.class_map == ""
    ns = p.parse_args(["--obj_ids", "1,5,6", "--shared_detector", "cfg/linemod.cfg,models/linemod.weights", "--class_map",
                       "1:0, 5:1,6:2"])
    assert shared_detector_arg(ns.shared_detector) == ("cfg/linemod.cfg", "models/linemod.weights")
    assert shared_detector_arg("a.cfg") == ("a.cfg", None)
    for bad in ("a.cfg,", ",w", "a,b,c"):
        with pytest.raises(ValueError):
            shared_detector_arg(bad)
    objs = id_list(ns.obj_ids)
    assert class_map(ns.class_map, objs) == {1: 0, 5: 1, 6: 2}
    # default: the position of the id in the sorted LineMod id list
    assert LINEMOD_IDS == sorted(LINEMOD_IDS) and len(LINEMOD_IDS) == 15
    assert class_map("", [1, 5, 6, 8, 9, 10, 11, 12]) == {1: 0, 5: 4, 6: 5, 8: 7, 9: 8, 10: 9, 11: 10, 12: 11}
    assert list(class_map("", [12, 1])) == [12, 1]                      # keyed in --obj_ids order
    assert class_map("7:3,5:0,1:9", [1, 5]) == {1: 9, 5: 0}              # extra entries are ignored
    for text, ids in (("1:0", [1, 5]), ("1:0,5:0", [1, 5]), ("1:0,1:1", [1]), ("1=0", [1]), ("1:-1", [1]), ("", [1, 16])):
        with pytest.raises(ValueError):
            class_map(text, ids)
    assert "args.shared_detector" in open(os.path.join(ROOT, "occlusion_evaluate.py")).read()


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_frame_sharded_ownership_covers_every_unit_once(world):
    frames, K = 7, 3
    owner = frame_sharded_owner(K, world)
    owners = [[r for r in range(world) if owner(u) == r] for u in range(frames * K)]
    assert all(len(o) == 1 for o in owners)                              # every unit exactly once
    for f in range(frames):
        assert {owners[f * K + oi][0] for oi in range(K)} == {f % world}  # a frame's units stay together, f % world
    per_rank = [sum(o[0] == r for o in owners) for r in range(world)]
    assert sum(per_rank) == frames * K and max(per_rank) - min(per_rank) <= K


def test_library_exports_the_scene_entry_points():
    _lib.lib()
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (bp_\w+)", syms))
    header = helpers.header_code()
    for name in SYMBOLS:
        assert name in exported, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES
    assert re.search(r"#define BP_MAX_SCENE_CLASSES 16\b", header) and _lib.MAX_SCENE_CLASSES == 16


def test_entry_points_fail_with_the_librarys_error_text():
    L = _lib.lib()
    ids = (C.c_int * 3)(0, 1, 2)
    h = C.c_void_p()
    assert L.bp_yolo_forward_select_classes(None, None, 1, 0.01, 80, C.cast(ids, C.c_void_p), 3, None, None, None) == -1
    assert b"null argument" in L.bp_last_error()
    assert L.bp_scene_create(None, None, C.cast(ids, C.c_void_p), 3, 480, 640, 0.01, 80, None, None, C.byref(h)) == -1
    assert b"null argument" in L.bp_last_error() and not h.value
    many = (C.c_int * 17)(*range(17))
    assert L.bp_scene_create(None, None, C.cast(many, C.c_void_p), 17, 480, 640, 0.01, 80, None, None, C.byref(h)) == -1
    assert b"1 to 16 class ids" in L.bp_last_error()
    assert L.bp_yolo_forward_select_classes(None, None, 1, 0.01, 80, C.cast(many, C.c_void_p), 17, None, None, None) == -1
    assert b"1 to 16 class ids" in L.bp_last_error()
    assert L.bp_yolo_forward_select_classes(None, None, 1, 0.01, 80, C.cast(ids, C.c_void_p), 0, None, None, None) == -1
    for rc in (L.bp_scene_set_pose_solver(None, 0, None, 0, None, 0, None), L.bp_scene_set_pose_ransac(None, 0, 1.0, 10, 0.99),
               L.bp_scene_prepare(None), L.bp_scene_run(None, 1, None)):
        assert rc == -1 and b"null argument" in L.bp_last_error()
    assert L.bp_scene_kernel_count(None) == -1 and L.bp_scene_results(None) is None and L.bp_scene_poses(None) is None
    L.bp_scene_destroy(None)


def _det15():
    d = Darknet("yolo/cfg/yolov3-single.cfg", reso=416)
    d.blocks = Cfg.parse_cfg_text(Cfg.yolov3_single_cfg_text(classes=15))
    d.net_info = d.blocks[0]
    return d


def test_class_lists_are_refused_with_a_clear_message():
    assert check_class_ids([7, 0, 12], 15) == [7, 0, 12]
    assert check_class_ids(range(15), 15, 80) == list(range(15))
    with pytest.raises(ValueError, match="17 class ids.*1 to 16"):
        check_class_ids(range(17), 80)
    with pytest.raises(ValueError, match="0 class ids"):
        check_class_ids([], 15)
    with pytest.raises(ValueError, match="duplicate class ids"):
        check_class_ids([3, 4, 3], 15)
    with pytest.raises(ValueError, match="class id 15 is not below the detector's class count 15"):
        check_class_ids([0, 15], 15)
    with pytest.raises(ValueError, match="class id 4 is not below the detector's class count 3"):
        check_class_ids([4], 15, num_classes=3)                         # the select compares min(num_classes, cfg) scores
    with pytest.raises(ValueError, match="class id -1"):
        check_class_ids([-1], 15)
    # the public surface refuses the same lists before it touches a device
    det = _det15()
    assert det.n_classes == 15 and Darknet("yolo/cfg/yolov3-single.cfg").n_classes == 1
    with pytest.raises(ValueError, match="class id 15"):
        det.forward_select_classes(None, [15])
    with pytest.raises(ValueError, match="duplicate"):
        det.forward_select_classes(None, [1, 1])
    with pytest.raises(ValueError, match="duplicate"):
        ScenePipeline(det, {1: None, 5: None}, {1: 2, 5: 2})
    with pytest.raises(ValueError, match="class id 20"):
        ScenePipeline(det, {1: None}, {1: 20})
    with pytest.raises(ValueError, match="1 to 16"):
        ScenePipeline(_det15(), {o: None for o in range(17)}, {o: o for o in range(17)}, num_classes=80)
    with pytest.raises(ValueError, match="no detector class"):
        ScenePipeline(det, {1: None, 5: None}, {1: 0})


def test_python_surface_needs_a_gpu():
    import torch
    if torch.cuda.is_available():
        return                      # with a GPU the same calls go on to build engines (tests/test_gpu_scene.py)
    with pytest.raises(_lib.BetaposeHipError, match="needs an AMD GPU"):
        ScenePipeline(_det15(), {1: None, 5: None}, {1: 0, 5: 4})
    with pytest.raises(_lib.BetaposeHipError, match="needs an AMD GPU"):
        _det15().forward_select_classes(None, [0, 4])


GATHER_WORKER = '''
import os, sys
import numpy as np
import torch.distributed as dist
sys.path.insert(0, %r)
from betapose_amd import dist as bpd
from betapose_amd.pipeline import frame_sharded_owner
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
rank, world = dist.get_rank(), dist.get_world_size()
frames, K = 3, 3                       # rank 0 owns frames 0 and 2: 6 of 9 units, more than ceil(9 / 2)
owner = frame_sharded_owner(K, world)
mine = [u for u in range(frames * K) if owner(u) == rank]
rec = np.array([[u, u * u, rank] for u in mine], np.float32).reshape(-1, 3)
out = bpd.gather_records(rec, mine, frames * K, max_local=-(-frames // world) * K)
if rank == 0:
    assert np.array_equal(out[:, 0], np.arange(frames * K)) and np.array_equal(out[:, 2], (np.arange(frames * K) // K) %% world)
    print("FRAME_GATHER_OK")
bpd.finalize()
'''


def test_two_rank_gather_of_frame_sharded_units(tmp_path):
    import socket
    import sys
    script = tmp_path / "worker.py"
    script.write_text(GATHER_WORKER % ROOT)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True))
    outs = [p.communicate(timeout=180)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "FRAME_GATHER_OK" in outs[0]
