"""Scenes of several targets on the host (betapose_amd/synth.py instance_masks, synthesize_multi): the
instance masks against a numpy restatement and against the renderer's own accumulation, the removal rule and its fixed
point, the tree, the labels of every object and the command line.  Every check is byte or integer equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import raster_common as rc  # noqa: E402
import synth_common as sc  # noqa: E402
import synth_multi_common as mc  # noqa: E402
from betapose_amd import _lib, annotate as A, metrics, sixd, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -------------------------------------------------------------------------------------------------- instance masks
@pytest.mark.parametrize("J", mc.OBJECTS)
@pytest.mark.parametrize("size", mc.SIZES)
def test_instance_masks_equal_their_restatement(size, J):
    alone, present = mc.random_stack(size, J)
    got, want = mc.host_instances(size, J), mc.numpy_instances(alone, present)
    for g, w, name in zip(got, want, ("ids", "depth", "stats")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    ids, depth, stats = got
    assert (stats[:, J - 1, :2] == 0).all() and (stats[:, J - 1, 2:] == -1).all()        # the object that covers no pixel
    if J > 1:
        assert stats[1, 0, 0] > 0 and stats[1, 0, 1] == 0 and (stats[1, 0, 6:] == -1).all() and (stats[1, 0, 2:6] >= 0).all()
        assert (ids[1] != 1).all() and (ids[0] == 1).any()                               # absent from scene 1 only
        ties = (alone[:, 0] == depth[0][None]) & (alone[:, 0] > 0)
        assert (ties.sum(axis=0) > 1).any()                                              # the stacks do hold exact ties
    assert not ids[2].any() and not depth[2].any() and (stats[2, :, 1] == 0).all() and (stats[2, :, 6:] == -1).all()


def test_present_defaults_to_every_object():
    alone, _ = mc.random_stack((48, 64), 3)
    a, b = synth.instance_masks(alone), synth.instance_masks(alone, np.ones((mc.IMAGES, 3), bool))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_entry_refuses_what_it_cannot_index():
    lib = _lib.lib()
    one = np.zeros(4, np.float32)
    u8, st = np.zeros(4, np.uint8), np.zeros(40, np.int32)
    call = lambda J, I, H, W: lib.bp_synth_instances_host(_lib.ptr(one), J, I, H, W, _lib.ptr(u8), _lib.ptr(u8), _lib.ptr(one), _lib.ptr(st))
    for args, word in (((0, 1, 2, 2), "J must lie"), ((33, 1, 2, 2), "J must lie"), ((1, 1, 4097, 4096), "2^24"), ((1, 0, 2, 2), "positive")):
        assert call(*args) == -1 and word in lib.bp_last_error().decode()
    assert call(1, 1, 2, 2) == 0
    with pytest.raises(ValueError):
        synth.instance_masks(np.zeros((2, 1, 4, 4), np.float64))
    with pytest.raises(ValueError):
        synth.instance_masks(np.zeros((2, 1, 4, 4), np.float32), np.ones((2, 1)))


@pytest.mark.parametrize("size", mc.SIZES)
def test_tie_goes_to_the_higher_object(size):
    """Objects 0 and 3 are one mesh at one pose: wherever both are drawn their depths are the same bits."""
    alone, _, _ = mc.rendered_stack(size)
    pair = np.ascontiguousarray(alone[[0, 3]])
    ids, depth, stats = synth.instance_masks(pair)
    assert set(np.unique(ids)) == {0, 2} and np.array_equal(depth, pair[1])
    assert (stats[:, 0, 1] == 0).all() and (stats[:, 0, 6:] == -1).all() and (stats[:, 0, 0] > 0).all()
    assert np.array_equal(stats[:, 0, 2:6], stats[:, 1, 2:6]) and np.array_equal(stats[:, 1, 2:6], stats[:, 1, 6:])
    assert np.array_equal(stats[:, 1, 0], stats[:, 1, 1]) and np.array_equal(stats[:, 0, 0], stats[:, 1, 0])


@pytest.mark.parametrize("size", mc.SIZES)
def test_full_stats_are_mask_boxes(size):
    alone, _, present = mc.rendered_stack(size)
    stats = synth.instance_masks(alone, present)[2]
    for j in range(alone.shape[0]):
        boxes, counts = A.mask_boxes(alone[j], rc.camera(size))
        assert np.array_equal(stats[:, j, 0], counts[:, 0]) and np.array_equal(stats[:, j, 2:6], boxes[:, 0])


@pytest.mark.parametrize("size", mc.SIZES)
def test_depth_and_colour_are_the_render_chain(size):
    """render_color(into=...) over the present objects in ascending j gives instance_masks' depth bit for bit, and at a
    pixel owned by object j the colour of object j rendered alone."""
    alone, poses, present = mc.rendered_stack(size)
    ids, depth, _ = synth.instance_masks(alone, present)
    K, objs = rc.camera(size), mc.render_objects()
    I = alone.shape[1]
    color, zbuf = np.zeros((I,) + tuple(size) + (3,), np.uint8), np.zeros((I,) + tuple(size), np.float32)
    for j, (v, f, c) in enumerate(objs):
        rows = np.flatnonzero(present[:, j])
        color, zbuf, _ = metrics.render_color(poses[rows, j], v, f, c, K, size, image_index=rows.astype(np.int32), images=I,
                                              into=(color, zbuf))
    assert zbuf.tobytes() == depth.tobytes()
    assert (ids == 4).any() and (ids == 1).any()            # the tie's winner, and the loser where the winner is absent
    for j, (v, f, c) in enumerate(objs):
        lone = metrics.render_color(poses[:, j], v, f, c, K, size)[0]
        own = ids == j + 1
        assert own.any() and np.array_equal(color[own], lone[own]), j


# ------------------------------------------------------------------------------------------------- synthesize_multi
def test_stream_zero_is_sample_poses_as_it_was():
    K, size = rc.camera(mc.MULTI_SIZE), mc.MULTI_SIZE
    a = synth.sample_poses(3, K, size, 0.05, 7, first_scene=2)
    assert a.tobytes() == synth.sample_poses(3, K, size, 0.05, 7, first_scene=2, stream=0).tobytes()
    assert a.tobytes() != synth.sample_poses(3, K, size, 0.05, 7, first_scene=2, stream=1).tobytes()
    s = mc.host_multi()
    radius = float(np.linalg.norm(mc.multi_meshes_metres()[0][0], axis=1).max())
    p = synth.sample_poses(4, K, size, radius, mc.MULTI_SEED)
    assert s["poses"][:, 0, :, :3].tobytes() == np.ascontiguousarray(p[..., :3]).tobytes()
    assert np.array_equal(s["t_mm"][:, 0], p[..., 3] * 1000.0) and np.array_equal(s["poses"][..., 3], s["t_mm"] * 0.001)


def test_multi_scenes_are_what_they_say():
    s = mc.host_multi()
    (H, W), J = mc.MULTI_SIZE, 4
    assert s["frames"].shape == (4, H, W, 3) and s["depth"].shape == (4, H, W) and s["depth"].dtype == np.uint16
    assert s["ids"].shape == (4, H, W) and s["ids"].dtype == np.uint8 and s["obj_ids"].tolist() == mc.MULTI_IDS
    for key, tail in (("poses", (3, 4)), ("t_mm", (3,)), ("box_full", (4,)), ("box_visible", (4,)), ("visib_fract", ()), ("px_all", ()),
                      ("px_visib", ()), ("present", ())):
        assert s[key].shape == (4, J) + tail, key
    pres, vf = s["present"], s["visib_fract"]
    # the three kinds the seed was chosen for
    assert (~pres).any() and (pres & (vf > 0) & (vf < 1)).any() and (pres & (vf == 1.0)).any()
    assert (s["px_visib"][pres].astype(np.float64) >= mc.MULTI_MIN_VISIB * s["px_all"][pres].astype(np.float64)).all()
    assert (s["px_all"][pres] > 0).all() and (s["px_visib"][~pres] == 0).all() and (s["box_visible"][~pres] == -1).all()
    for j in range(J):
        assert np.array_equal((s["ids"] == j + 1).sum(axis=(1, 2)), s["px_visib"][:, j])
    assert np.array_equal(s["visib_fract"], s["px_visib"] / np.maximum(s["px_all"], 1))
    # the depth image is the owners' depth through the noiseless sensor: covered exactly where somebody owns the pixel
    assert np.array_equal(s["depth"] > 0, s["ids"] > 0)


def test_one_round_of_removal_is_a_fixed_point():
    """Running the rule again on the returned scenes drops nothing, and no survivor lost a pixel to the removal."""
    s = mc.host_multi()
    ms, K = mc.multi_meshes_metres(), rc.camera(mc.MULTI_SIZE)
    alone = np.stack([metrics.render_depth(s["poses"][:, j], ms[j][0], ms[j][1], K, mc.MULTI_SIZE)[0] for j in range(4)])
    before = synth.instance_masks(alone)[2]
    ids, _, after = synth.instance_masks(alone, s["present"])
    assert np.array_equal(~synth.below_visibility(before, mc.MULTI_MIN_VISIB), s["present"])
    assert np.array_equal(ids, s["ids"]) and np.array_equal(after[..., 1], s["px_visib"]) and np.array_equal(after[..., 0], s["px_all"])
    assert not synth.below_visibility(after, mc.MULTI_MIN_VISIB)[s["present"]].any()
    assert (after[..., 1][s["present"]] >= before[..., 1][s["present"]]).all()
    assert (after[..., 1][s["present"]] > before[..., 1][s["present"]]).any()           # somebody was uncovered


def test_multi_chunks_concatenate_to_the_whole(monkeypatch):
    whole = mc.host_multi()
    parts = [mc.synthesize_multi(2), mc.synthesize_multi(2, first_scene=2)]
    for key, want in whole.items():
        got = parts[0][key] if key == "obj_ids" else np.concatenate([parts[0][key], parts[1][key]])
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), key
    # ... and the function's own chunks: a stack bound of one scene's floats makes it take the scenes one by one
    monkeypatch.setattr(synth, "MULTI_STACK_FLOATS", 4 * mc.MULTI_SIZE[0] * mc.MULTI_SIZE[1])
    for key, got in mc.synthesize_multi(4).items():
        assert got.tobytes() == whole[key].tobytes(), key


def test_synthesize_multi_checks_its_arguments():
    ms, K = mc.multi_meshes_metres(), rc.camera(mc.MULTI_SIZE)
    with pytest.raises(ValueError):
        synth.synthesize_multi(ms, K, mc.MULTI_SIZE, 1, 0, obj_ids=[1, 2, 3])
    with pytest.raises(ValueError):
        synth.synthesize_multi(ms, K, mc.MULTI_SIZE, 1, 0, obj_ids=[1, 2, 2, 3])
    with pytest.raises(ValueError):
        synth.synthesize_multi(ms[:1] * 33, K, mc.MULTI_SIZE, 1, 0)


# ------------------------------------------------------------------------------------------------------------ files
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    base = str(tmp_path_factory.mktemp("multi_tree"))
    synth.write_scene_tree(base, 2, mc.host_multi(), mc.multi_meshes(), rc.camera(mc.MULTI_SIZE), 0.001)
    return base


def test_multi_tree_round_trip(tree):
    import yaml
    s = mc.host_multi()
    bench = sixd.load_sixd(tree, 2, load_depth=True)
    assert len(bench.frames) == 4 and np.array_equal(bench.cam, rc.camera(mc.MULTI_SIZE))
    with open(os.path.join(tree, "test", "02", "gt.yml")) as f:
        gt = yaml.safe_load(f)
    from betapose_amd.frame_loader import decode_png
    for i, fr in enumerate(bench.frames):
        present = [j for j in range(4) if s["present"][i, j]]
        assert [g[0] for g in fr.gt] == [mc.MULTI_IDS[j] for j in present]               # all rows of the frame, in order
        for g, row, j in zip(fr.gt, gt[i], present):
            assert g[1][:3].tobytes() == s["poses"][i, j].tobytes()
            xmin, xmax, ymin, ymax = (int(v) for v in s["box_full"][i, j])
            assert list(g[2]) == [xmin, ymin, xmax - xmin, ymax - ymin] == row["obj_bb"]
            xmin, xmax, ymin, ymax = (int(v) for v in s["box_visible"][i, j])
            assert row["obj_bb_visib"] == [xmin, ymin, xmax - xmin, ymax - ymin]
            assert row["visib_fract"] == s["visib_fract"][i, j]
            assert (row["px_count_all"], row["px_count_visib"]) == (s["px_all"][i, j], s["px_visib"][i, j])
        assert np.array_equal(fr.depth, s["depth"][i])
        with open(os.path.join(tree, "test", "02", "rgb", "%04d.png" % i), "rb") as f:
            assert np.array_equal(decode_png(f.read()), s["frames"][i])
        from PIL import Image
        mask = np.asarray(Image.open(os.path.join(tree, "test", "02", "mask", "%04d.png" % i)))
        assert mask.dtype == np.uint8 and mask.shape == mc.MULTI_SIZE
        assert np.array_equal(mask, np.array([0] + mc.MULTI_IDS, np.uint8)[s["ids"][i]])
    assert sorted(os.listdir(os.path.join(tree, "models"))) == ["models_info.yml"] + ["obj_%02d.ply" % o for o in mc.MULTI_IDS]


def test_a_tree_of_one_target_is_the_bytes_it_was(tmp_path):
    """write_scene_tree of synthesize_scenes' output: the digest recorded on the commit before this feature."""
    scenes = sc.synthesize(4)
    assert "ids" not in scenes
    base = str(tmp_path / "t")
    synth.write_scene_tree(base, 1, scenes, sc.scene_meshes(), rc.camera(sc.SCENES_SIZE), 0.001)
    assert not os.path.exists(os.path.join(base, "test", "01", "mask"))
    assert mc.tree_digest(base) == mc.SINGLE_TREE_DIGEST


def test_annotator_picks_each_object_out_of_the_tree(tree):
    s = mc.host_multi()
    bench = sixd.load_sixd(tree, 2, load_depth=True)
    for j, oid in ((0, 1), (2, 6)):
        v, f = metrics.load_ply_mesh(os.path.join(tree, "models", "obj_%02d.ply" % oid))
        model = metrics.Model3D()
        model.vertices = v * bench.scale_to_meters
        bench.models["%02d" % oid] = model
        ann = A.annotate_sequence(bench, oid, model.vertices[::5], f, use_depth=True, size=mc.MULTI_SIZE)
        rows = np.flatnonzero(s["present"][:, j])
        assert 0 < len(rows) < 4 and ann["frames"].tolist() == rows.tolist()             # only that object's frames
        assert np.array_equal(ann["box_full"], s["box_full"][rows, j])
        assert ann["kp_label"].shape == (len(rows), len(model.vertices[::5]), 2)


def test_labels_are_the_reference_scripts_arithmetic():
    WIDTH, HEIGHT = 640, 480
    rows = [{"obj_id": 1, "obj_bb": [10, 20, 31, 45], "obj_bb_visib": [12, 20, 5, 7]},
            {"obj_id": 7, "obj_bb": [0, 0, 639, 479]},
            {"obj_id": 15, "obj_bb": [601.5, 3, 7, 1], "obj_bb_visib": [-1, -1, 0, 0]}]
    want = []
    for gt in rows:                                         # gt_multi_object.py's loop body
        obj_id = gt["obj_id"] - 1
        bbox = list(gt["obj_bb"])
        bbox[0] = (bbox[0] + bbox[2] / 2) / WIDTH
        bbox[1] = (bbox[1] + bbox[3] / 2) / HEIGHT
        bbox[2] = bbox[2] / WIDTH
        bbox[3] = bbox[3] / HEIGHT
        want.append("%d %f %f %f %f" % (obj_id, bbox[0], bbox[1], bbox[2], bbox[3]))
    assert A.darknet_labels_multi(rows, {i: i - 1 for i in range(1, 16)}) == want
    assert want[0] == "0 0.039844 0.088542 0.048438 0.093750"
    assert rows[0]["obj_bb"] == [10, 20, 31, 45]                                        # the rows are not written to
    assert A.darknet_labels_multi(rows, {15: 0, 1: 1}) == ["1" + want[0][1:], "0" + want[2][2:]]   # row order, mapped, 7 left out
    assert A.darknet_labels_multi(rows, {1: 0}, box="visible") == ["0 %f %f %f %f" % (14.5 / 640, 23.5 / 480, 5 / 640, 7 / 480)]
    with pytest.raises(ValueError):
        A.darknet_labels_multi(rows, {7: 0}, box="visible")
    with pytest.raises(ValueError):
        A.darknet_labels_multi(rows, {7: 0}, box="both")


@pytest.mark.parametrize("box", ["full", "visible"])
def test_exported_detector_set_feeds_the_loader(tree, tmp_path, box):
    from betapose_amd.yolo_map import read_data_cfg
    from betapose_amd.yolo_train import YoloSampleLoader
    s = mc.host_multi()
    class_of = {1: 2, 5: 0, 6: 3, 9: 1}
    annot, out = str(tmp_path / "annot"), str(tmp_path / "set")
    split = A.write_multi_labels(tree, 2, annot, class_of, 3, seed=1, box=box)
    assert sorted(split["train"] + split["eval"]) == [0, 1, 2, 3] and len(split["train"]) == 3
    lists = synth.export_detector_set(tree, 2, annot, out)
    opts = read_data_cfg(lists["data"])
    assert opts["classes"] == 4 and opts["train"] == lists["train"] and opts["valid"] == lists["eval"]
    assert set(opts) >= {"classes", "train", "valid", "names", "backup"}
    with open(opts["names"]) as f:
        assert f.read().split() == ["obj_05", "obj_09", "obj_01", "obj_06"]
    loader = YoloSampleLoader(opts["train"], batch=4, net_size=(96, 96), classes=4, train=False, threads=1)
    (inps, truth), = list(loader)
    assert inps.shape == (3, 3, 96, 96) and truth.shape == (3, 90, 5)
    H, W = mc.MULTI_SIZE
    key = "box_full" if box == "full" else "box_visible"
    for k, nr in enumerate(split["train"]):
        present = [j for j in range(4) if s["present"][nr, j]]
        classes = [class_of[mc.MULTI_IDS[j]] for j in present]
        got = truth[k, :len(present), 4].tolist()           # (the loader shuffles a frame's boxes, as Darknet does)
        assert sorted(got) == sorted(classes) and not truth[k, len(present):].any()
        for j, c in zip(present, classes):
            r = got.index(c)
            xmin, xmax, ymin, ymax = s[key][nr, j].astype(np.float64)
            assert np.allclose(truth[k, r, :4], [(xmin + xmax) / 2 / W, (ymin + ymax) / 2 / H, (xmax - xmin) / W, (ymax - ymin) / H], atol=1e-6)
    # a benchmark (sixd.load_sixd) carries the full boxes only
    bench = sixd.load_sixd(tree, 2)
    other = str(tmp_path / "annot_bench")
    if box == "full":
        A.write_multi_labels(bench, 2, other, class_of, 3, seed=1, box=box, image_size=mc.MULTI_SIZE)
        for nr in range(4):
            assert open(os.path.join(other, "labels", "%04d.txt" % nr)).read() == open(os.path.join(annot, "labels", "%04d.txt" % nr)).read()
    else:
        with pytest.raises(ValueError):
            A.write_multi_labels(bench, 2, other, class_of, 3, seed=1, box=box, image_size=mc.MULTI_SIZE)


def test_detector_trains_on_the_exported_set(tree, tmp_path):
    """The chain's last link on the host twins: two iterations of a four-class net on the exported set, to a .weights file."""
    import io
    import darknet_train_common as dc
    sys.path.insert(0, ROOT)
    from train_detector import train_detector
    class_of = {o: c for c, o in enumerate(mc.MULTI_IDS)}
    annot, out = str(tmp_path / "annot"), str(tmp_path / "set")
    A.write_multi_labels(tree, 2, annot, class_of, 4, seed=0)
    data = synth.export_detector_set(tree, 2, annot, out)["data"]
    cfg = str(tmp_path / "tiny4.cfg")
    with open(cfg, "w") as f:
        f.write(dc.tiny_cfg(32, 24, 2, 1, 4, dc.NET_A + "jitter=.3\nhue=.1\nsaturation=1.5\nexposure=1.5\n"))
    log = io.StringIO()
    train_detector(data, cfg, max_batches=2, device="cpu", out=log)
    assert log.getvalue().count("avg loss") == 2 and "nan" not in log.getvalue()
    assert os.path.getsize(os.path.join(out, "backup", "tiny4_final.weights")) > 0


# -------------------------------------------------------------------------------------------------------------- CLI
def _run(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "synthesize.py")] + args, capture_output=True, text=True, timeout=300)


def _write_meshes(folder):
    paths = {}
    for oid, m in mc.multi_meshes().items():
        paths[oid] = os.path.join(str(folder), "m%02d.ply" % oid)
        synth._write_mesh_ply(paths[oid], m[0], m[1], m[2])
    return paths


def test_command_line_writes_the_multi_object_tree(tmp_path):
    paths = _write_meshes(tmp_path)
    out, det = str(tmp_path / "tree"), str(tmp_path / "det")
    r = _run(["--models", ",".join(paths[o] for o in mc.MULTI_IDS), "--obj_ids", ",".join(str(o) for o in mc.MULTI_IDS), "--seq", "2",
              "--frames", "3", "--out", out, "--size", "48x64", "--camera", "60,60,31.5,23.5", "--seed", str(mc.MULTI_SEED),
              "--detector_set", det, "--label_box", "visible", "--class_map", "1:0,5:1,6:2,9:3"])
    assert r.returncode == 0, r.stderr
    s = synth.synthesize_multi(mc.multi_meshes_metres(), rc.camera(mc.MULTI_SIZE), mc.MULTI_SIZE, 3, mc.MULTI_SEED, obj_ids=mc.MULTI_IDS)
    bench = sixd.load_sixd(out, 2, load_depth=True)
    assert len(bench.frames) == 3
    for i, fr in enumerate(bench.frames):
        assert [g[0] for g in fr.gt] == [o for j, o in enumerate(mc.MULTI_IDS) if s["present"][i, j]]
        assert np.array_equal(fr.depth, s["depth"][i])
    assert sorted(os.listdir(os.path.join(out, "test", "02", "mask"))) == ["%04d.png" % i for i in range(3)]
    from betapose_amd.yolo_map import read_data_cfg
    opts = read_data_cfg(os.path.join(det, "obj.data"))
    assert opts["classes"] == 4 and len(open(opts["train"]).read().split()) == 3 and open(opts["valid"]).read() == ""
    for p in open(opts["train"]).read().split():
        assert os.path.exists(p) and os.path.exists(p[:-4] + ".txt")


def test_command_line_of_one_target_is_unchanged(tmp_path):
    m = sc.scene_meshes()
    ply, occ = str(tmp_path / "obj_01.ply"), str(tmp_path / "occ.ply")
    synth._write_mesh_ply(ply, m[1][0], m[1][1], m[1][2])
    synth._write_mesh_ply(occ, m[2][0], m[2][1])
    out = str(tmp_path / "tree")
    r = _run(["--model", ply, "--occluders", occ, "--out", out] + mc.SINGLE_CLI_ARGS)
    assert r.returncode == 0, r.stderr
    assert mc.tree_digest(out) == mc.SINGLE_CLI_DIGEST
    for args in ([], ["--model", ply, "--models", ply, "--obj_ids", "1"]):
        r = _run(args + ["--out", out])
        assert r.returncode != 0 and "exactly one of --model" in r.stderr
    r = _run(["--models", ply + "," + occ, "--obj_ids", "1", "--out", out])
    assert r.returncode != 0 and "--obj_ids" in r.stderr
