"""Device-side stages around the networks, through the C-ABI: Pillow-exact bicubic resize (a1),
crop (a6/a7), the fused hipGraph pipeline (a1..a9) and its host tail (a9..a11), against the
reference golden vectors and the oracle.  Integer results exact; floats within stated tolerance."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import helpers  # noqa: E402
from betapose_amd import ops, synth  # noqa: E402
from betapose_amd.darknet import Darknet  # noqa: E402
from betapose_amd.kpd import FastPoseHIP  # noqa: E402
from betapose_amd.pipeline import FramePipeline, finish_record  # noqa: E402
from oracle import post_ref  # noqa: E402


@pytest.mark.parametrize("size", [(480, 640, 416, 416), (480, 640, 320, 256), (100, 37, 64, 80), (416, 416, 416, 416)])
def test_resize_is_pillow_exact(cuda, size):
    H, W, oh, ow = size
    rng = np.random.Generator(np.random.PCG64(H * 1000 + W))
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    got = ops.resize_bicubic(torch.from_numpy(frames).to(cuda), oh, ow, swap_rb=False, want="u8").cpu().numpy()
    for b in range(2):
        ref = np.asarray(Image.fromarray(frames[b]).resize((ow, oh), 3))
        assert np.array_equal(got[b], ref), "max diff %d" % int(np.abs(got[b].astype(int) - ref.astype(int)).max())


def test_resize_matches_reference_input_path(cuda):
    """BGR frame -> RGB /255 NHWC == transforms.Resize((416,416), 3) + ToTensor of the reference (dataloader.py:94-99)."""
    pipe = helpers.golden("pipeline.npz")
    fr = helpers.frames()[0]
    got = ops.resize_bicubic(torch.from_numpy(fr[None]).to(cuda), 416, 416, swap_rb=True, want="f32").cpu()
    nchw = got.permute(0, 3, 1, 2).contiguous()
    assert np.array_equal(nchw.numpy().ravel()[pipe["in_samp"]], pipe["f0_yolo_in_samp"])
    assert int(torch.round(nchw * 255).long().sum()) == int(pipe["f0_yolo_in_u8sum"])


def test_crop_matches_reference(cuda):
    pipe = helpers.golden("pipeline.npz")
    n = int(pipe["n_frames"])
    frames = np.stack(helpers.frames(n))
    boxes = np.concatenate([pipe["f%d_boxes" % i] for i in range(n)]).astype(np.float32)
    inps, pts = ops.crop(torch.from_numpy(frames).to(cuda), boxes=torch.from_numpy(boxes).to(cuda))
    inps, pts = inps.cpu(), pts.cpu().numpy()
    for i in range(n):
        k = "f%d_" % i
        np.testing.assert_array_equal(pts[i, 0:2], pipe[k + "pt1"][0])      # float window, exact
        np.testing.assert_array_equal(pts[i, 2:4], pipe[k + "pt2"][0])
        np.testing.assert_allclose(inps[i].numpy().ravel()[pipe["crop_samp"]], pipe[k + "crop_samp"], atol=2e-6)
        assert abs(float(inps[i].double().sum()) - float(pipe[k + "crop_sum"])) < 0.05


@pytest.mark.parametrize("box", [(0.0, 0.0, 60.0, 50.0), (600.0, 430.0, 639.0, 479.0), (-20.0, 100.0, 700.0, 130.0),
                                 (300.0, 200.0, 302.0, 203.0), (10.5, 20.25, 90.75, 260.5), (100.0, 50.0, 201.0, 400.0)])
def test_crop_edge_boxes_vs_oracle(cuda, box):
    """Borders, degenerate and clamped boxes (the cases crop_from_dets guards, dataloader.py:817-823)."""
    fr = helpers.frames()[1]
    b = torch.tensor([box], dtype=torch.float32)
    ref, pt1, pt2 = post_ref.crop_from_dets_frame(fr, b)
    got, pts = ops.crop(torch.from_numpy(fr[None]).to(cuda), boxes=b.to(cuda))
    np.testing.assert_array_equal(pts.cpu().numpy()[0, :4], np.r_[pt1.numpy()[0], pt2.numpy()[0]])
    assert float((got.cpu() - ref).abs().max()) <= 2e-6


def test_crop_random_box_sweep_vs_oracle(cuda):
    """240 seeded boxes of every flavour -- tiny, huge, partly or wholly outside the frame, fractional corners, the
    w == 100 px pad-rule boundary -- in one batched launch against the oracle's per-box crop_from_dets."""
    rng = np.random.default_rng(42)
    fr = helpers.frames()[2]
    boxes = []
    for _ in range(200):
        cx, cy = rng.uniform(-50, 690), rng.uniform(-50, 530)
        w, h = np.exp(rng.uniform(np.log(2), np.log(700))), np.exp(rng.uniform(np.log(2), np.log(500)))
        boxes.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
    for w in (99.0, 99.999, 100.0, 100.001, 101.0):                    # scaleRate switches at width 100 (dataloader.py:811)
        for x0 in (0.0, 33.3, 539.5, 560.0):
            boxes.append([x0, 120.25, x0 + w, 300.5])
    for _ in range(20):                                                 # integer-cornered boxes
        x0, y0 = rng.integers(0, 600), rng.integers(0, 440)
        boxes.append([float(x0), float(y0), float(x0 + rng.integers(1, 200)), float(y0 + rng.integers(1, 200))])
    b = torch.tensor(boxes, dtype=torch.float32)
    n = len(boxes)
    got, pts = ops.crop(torch.from_numpy(np.repeat(fr[None], n, 0)).to(cuda), boxes=b.to(cuda))
    got, pts = got.cpu(), pts.cpu().numpy()
    worst = 0.0
    for i in range(n):
        ref, pt1, pt2 = post_ref.crop_from_dets_frame(fr, b[i:i + 1])
        np.testing.assert_array_equal(pts[i, :4], np.r_[pt1.numpy()[0], pt2.numpy()[0]], err_msg=str(boxes[i]))
        worst = max(worst, float((got[i] - ref[0]).abs().max()))
    assert worst <= 2e-6, worst


@pytest.fixture(scope="module")
def engines(cuda):
    det = Darknet("yolo/cfg/yolov3-single.cfg", reso=416, max_batch=4).load_stream(helpers.yolo_stream()).cuda()
    pose = FastPoseHIP(helpers.kpd_state_dict(), max_batch=4).cuda()
    return det, pose


@pytest.mark.parametrize("use_graph", [False, True])
def test_pipeline_matches_reference_golden(engines, cuda, use_graph):
    """Frame in -> record out, one launch sequence / one hipGraph; everything the reference's stage classes
    produced for the same frames (tests/golden/pipeline.npz)."""
    det, pose = engines
    pipe = helpers.golden("pipeline.npz")
    fp = FramePipeline(det, pose, 480, 640, batch=1, use_graph=use_graph, keep_heatmaps=True)
    kp3d = synth.synth_kp3d(50)
    for rep in range(2):   # second pass replays the captured graph
        for i, fr in enumerate(helpers.frames(int(pipe["n_frames"]))):
            k = "f%d_" % i
            rec = fp.run(fr)[0]
            out = finish_record(rec, "%04d.png" % i, kp3d, synth.CAM_K)
            assert out["yolo_index"] == int(pipe[k + "obj_argmax"])
            np.testing.assert_allclose(out["boxes"], pipe[k + "boxes"], rtol=3e-5, atol=2e-3)
            np.testing.assert_allclose(out["scores"], pipe[k + "scores"], atol=2e-5)
            np.testing.assert_allclose(rec[8:12], np.r_[pipe[k + "pt1"][0], pipe[k + "pt2"][0]], rtol=3e-5, atol=2e-3)
            kp = rec[16:].reshape(50, 6)
            assert np.array_equal(kp[:, 0].copy().view(np.int32), pipe[k + "kp_idx"])
            assert np.abs(kp[:, 1] - pipe[k + "kp_max"]).max() <= 2e-4
            hm = fp.heatmaps.cpu().numpy()
            assert np.abs(hm.ravel()[pipe["hm_samp"]] - pipe[k + "hm_samp"]).max() <= 2e-4
            assert len(out["result"]) == int(pipe[k + "nms_n"]) == 1
            np.testing.assert_allclose(out["result"][0]["keypoints"], pipe[k + "nms_kp"], rtol=1e-4, atol=5e-3)
            np.testing.assert_allclose(out["result"][0]["kp_score"], pipe[k + "nms_score"], atol=2e-4)
            # pose: the product's solver on the pipeline's own key points against the oracle's independent restatement
            # of cv2.solvePnP(SOLVEPNP_ITERATIVE) on the same points (random-weight key points are no consistent
            # projection: this is the ill-posed input class; the well-posed ones are in tests/test_pnp.py)
            R, t = out["cam_R"], out["cam_t"]
            Ro, to = post_ref.solve_pnp_iterative_ref(kp3d, out["result"][0]["keypoints"], synth.CAM_K)
            assert np.abs(R - Ro).max() < 1e-5 and np.abs(t - to).max() < 1e-5 and abs(np.linalg.det(R) - 1) < 1e-9
    if use_graph:
        assert fp.kernel_count() > 100


def test_pipeline_batch_equals_single(engines, cuda):
    det, pose = engines
    frames = np.stack(helpers.frames(3))
    fb = FramePipeline(det, pose, 480, 640, batch=3, use_graph=True)
    recb = fb.run(frames)
    f1 = FramePipeline(det, pose, 480, 640, batch=1, use_graph=True)
    for i in range(3):
        r1 = f1.run(frames[i])[0]
        assert r1[:1].view(np.int32)[0] == recb[i, :1].view(np.int32)[0]
        a, b = r1[16:].reshape(50, 6), recb[i, 16:].reshape(50, 6)
        assert np.array_equal(a[:, 0].copy().view(np.int32), b[:, 0].copy().view(np.int32))
        assert np.abs(a[:, 1:] - b[:, 1:]).max() <= 2e-4


def test_pipeline_fixed_box(engines, cuda):
    det, pose = engines
    fp = FramePipeline(det, pose, 480, 640, batch=1, use_graph=True)
    fp.set_fixed_box([220, 140, 420, 340])
    rec = fp.run(helpers.frames()[0])[0]
    np.testing.assert_allclose(rec[12:16], [220, 140, 420, 340])
    fp.set_fixed_box(None)
    rec2 = fp.run(helpers.frames()[0])[0]
    assert not np.allclose(rec2[12:16], [220, 140, 420, 340])


def test_select_random_predictions_vs_oracle(cuda):
    """dynamic_write_results on 60 seeded prediction tensors against the oracle's write_results: multi-class rows whose
    arg-max class is not 0 (dropped by the reference), ties on objectness (first index wins), images without any row
    above the threshold, batches mixing all of these."""
    from betapose_amd.yolo_util import dynamic_write_results
    from oracle import yolo_ref
    rng = np.random.default_rng(7)
    for trial in range(60):
        B = int(rng.integers(1, 5))
        rows = int(rng.choice([17, 507, 2535]))
        ncls = int(rng.choice([1, 3]))
        pred = np.zeros((B, rows, 5 + ncls), np.float32)
        pred[..., 0:2] = rng.uniform(0, 416, (B, rows, 2))
        pred[..., 2:4] = rng.uniform(2, 300, (B, rows, 2))
        pred[..., 4] = rng.uniform(0, 1, (B, rows)) ** 3
        pred[..., 5:] = rng.uniform(0, 1, (B, rows, ncls))
        conf = float(rng.choice([0.01, 0.5, 0.9]))
        if trial % 4 == 0:                                    # an image with nothing above the threshold
            pred[0, :, 4] *= conf * 0.5
        tied = trial % 5 == 0
        if tied:                                              # exact ties on the best objectness
            b = int(rng.integers(0, B))
            top = pred[b, :, 4].max()
            for j in rng.choice(rows, 3, replace=False):
                pred[b, j, 4] = top
        t = torch.from_numpy(pred)
        want = yolo_ref.write_results(t.clone(), conf, 80)
        got = dynamic_write_results(t.to(cuda), conf, 80)
        if isinstance(want, int):
            assert isinstance(got, int) and got == 0, (trial, got)
            continue
        assert not isinstance(got, int), trial
        assert got.shape == want.shape, (trial, got.shape, want.shape)
        g, w_ = got.cpu().numpy(), want.numpy()
        if not tied:
            np.testing.assert_allclose(g, w_, rtol=1e-6, atol=1e-5, err_msg="trial %d" % trial)
            continue
        # exact ties: the reference ranks with an unstable torch.sort (util.py:175-181), so WHICH of the tied rows it
        # returns is unspecified; here the first one in row order wins.  Both must return a tied row of class 0.
        np.testing.assert_allclose(g[:, [0, 5]], w_[:, [0, 5]], rtol=1e-6, err_msg="trial %d" % trial)
        for r in g:
            img = pred[int(r[0])]
            ok = (img[:, 4] == r[5]) & (img[:, 5:].argmax(1) == 0)
            cand = img[ok]
            corners = np.stack([cand[:, 0] - cand[:, 2] / 2, cand[:, 1] - cand[:, 3] / 2, cand[:, 0] + cand[:, 2] / 2,
                                cand[:, 1] + cand[:, 3] / 2], 1)
            d = np.abs(corners - r[1:5]).max(1)
            assert d.min() < 1e-3, trial
            assert d.argmin() == 0, "first tied row in row order must win (trial %d)" % trial


def test_heatmap_argmax_random_maps_vs_oracle(cuda):
    """The arg-max half of getPrediction on seeded heat-maps with the awkward cases planted: maxima on every border and
    corner (no quarter-pixel shift there), exact ties (first pixel wins, as torch.max on CPU), maps that are <= 0
    everywhere (key point zeroed), flat neighbourhoods (sign(0) = 0).  Compared through the whole decode against the
    oracle's get_prediction."""
    from betapose_amd.eval import decode_keypoints
    rng = np.random.default_rng(11)
    n, K, H, W = 6, 50, 80, 64
    hm = rng.normal(0, 0.3, (n, K, H, W)).astype(np.float32)
    for k, (y, x) in enumerate([(0, 0), (0, 63), (79, 0), (79, 63), (0, 30), (79, 31), (40, 0), (41, 63)]):
        hm[0, k, y, x] = 5.0                                   # border / corner maxima
    for k in range(8, 16):                                     # exact ties: two equal maxima, the earlier pixel wins
        a, b = sorted(rng.choice(H * W, 2, replace=False))
        hm[0, k].reshape(-1)[[a, b]] = 4.0
    hm[1, :10] = -np.abs(hm[1, :10]) - 0.01                    # all negative
    hm[1, 10:12] = 0.0                                         # all zero: maxval == 0 -> zeroed too
    for k in range(12, 20):                                    # interior maximum with equal left/right or up/down
        y, x = int(rng.integers(1, H - 1)), int(rng.integers(1, W - 1))
        hm[1, k, y, x] = 6.0
        hm[1, k, y, x - 1] = hm[1, k, y, x + 1] = 1.5
        hm[1, k, y - 1, x], hm[1, k, y + 1, x] = 0.5, 2.5
    pt1 = rng.uniform(0, 200, (n, 2)).astype(np.float32)
    pt2 = pt1 + rng.uniform(20, 300, (n, 2)).astype(np.float32)
    t = torch.from_numpy(hm)
    kp = ops.heatmap_argmax(t.to(cuda)).cpu().numpy()
    idx = kp[..., 0].copy().view(np.int32)
    assert np.array_equal(idx, hm.reshape(n, K, -1).argmax(2))
    got_hm, got_img, got_max = decode_keypoints(kp, pt1, pt2)
    ref_hm, ref_img, ref_max = post_ref.get_prediction(t, torch.from_numpy(pt1), torch.from_numpy(pt2))
    np.testing.assert_array_equal(got_hm, ref_hm.numpy())
    np.testing.assert_allclose(got_img, ref_img.numpy(), rtol=0, atol=2e-4)
    np.testing.assert_array_equal(got_max, ref_max.numpy())
    assert np.all(got_hm[1, :12] == np.float32(0.2))           # zeroed key points (then the +0.2 of eval.py:131)
    # degenerate input must stay in bounds
    bad = torch.full((1, 2, H, W), float("-inf"))
    out = ops.heatmap_argmax(bad.to(cuda)).cpu().numpy()
    assert np.all(out[..., 0].copy().view(np.int32) == 0)


def test_pipeline_frame_without_detection(engines, cuda):
    """No candidate above the confidence: the record carries index -1, the host tail forwards the frame with
    boxes=None exactly as the reference does (dataloader.py:344-349), and the next frame is unaffected."""
    from betapose_amd.pipeline import finish_record
    det, pose = engines
    fr = helpers.frames()[0]
    strict = FramePipeline(det, pose, 480, 640, batch=1, confidence=0.9999)
    rec = strict.run(fr)[0]
    assert int(rec[:1].view(np.int32)[0]) == -1
    out = finish_record(rec, "0000.png", synth.synth_kp3d(50), synth.CAM_K)
    assert out["boxes"] is None and out["result"] == [] and out["cam_R"] == []
    normal = FramePipeline(det, pose, 480, 640, batch=1, confidence=0.01)
    rec2 = normal.run(fr)[0]
    assert int(rec2[:1].view(np.int32)[0]) == int(helpers.golden("pipeline.npz")["f0_obj_argmax"])


def test_crop_and_select_match_reference_edge_goldens(cuda):
    """The HIP crop and select kernels directly against the REFERENCE's outputs on the edge-case fixtures
    (tests/golden/edges.npz, tools/make_golden_edges.py)."""
    from betapose_amd.yolo_util import dynamic_write_results
    e = helpers.golden("edges.npz")
    fr = synth.synth_frame(int(e["crop_frame_seed"]))
    boxes = torch.from_numpy(e["crop_boxes"])
    n = len(boxes)
    got, pts = ops.crop(torch.from_numpy(np.repeat(fr[None], n, 0)).to(cuda), boxes=boxes.to(cuda))
    got, pts = got.cpu().reshape(n, -1), pts.cpu().numpy()
    np.testing.assert_array_equal(pts[:, 0:2], e["crop_pt1"])
    np.testing.assert_array_equal(pts[:, 2:4], e["crop_pt2"])
    assert np.abs(got.numpy()[:, e["crop_samp_idx"]] - e["crop_samples"]).max() <= 2e-6
    assert np.abs(got.double().sum(1).numpy() - e["crop_sum"]).max() < 0.05
    for t in range(int(e["sel_n"])):
        want = e["sel%d_out" % t]
        res = dynamic_write_results(torch.from_numpy(e["sel%d_pred" % t]).to(cuda), float(e["sel%d_conf" % t]), 80)
        if len(want) == 0:
            assert isinstance(res, int) and res == 0, t
        else:
            np.testing.assert_allclose(res.cpu().numpy(), want, rtol=1e-6, atol=1e-5, err_msg="case %d" % t)
    # arg-max kernel + host decode against the reference's getPrediction on the planted heat-maps
    from betapose_amd.eval import decode_keypoints
    hm = torch.from_numpy(e["gpe_hms"].astype(np.float32))
    kp = ops.heatmap_argmax(hm.to(cuda)).cpu().numpy()
    a, b, c = decode_keypoints(kp, e["gpe_pt1"], e["gpe_pt2"])
    np.testing.assert_array_equal(a, e["gpe_preds_hm"])
    np.testing.assert_allclose(b, e["gpe_preds_img"], rtol=0, atol=1e-4)
    np.testing.assert_array_equal(c, e["gpe_maxval"])


def test_crop_from_dets_reference_signature(cuda):
    """dataloader.crop_from_dets(img, boxes, inps, pt1, pt2) with the reference's arguments and side effects, against the
    reference's own outputs on the edge-box fixture."""
    from betapose_amd.dataloader import crop_from_dets
    from betapose_amd.img import im_to_torch
    e = helpers.golden("edges.npz")
    fr = synth.synth_frame(int(e["crop_frame_seed"]))
    idx = [0, 7, 19, 41, 50, 63]
    boxes = torch.from_numpy(e["crop_boxes"][idx])
    img = im_to_torch(np.ascontiguousarray(fr[:, :, ::-1]))
    before = img.clone()
    inps, pt1, pt2 = torch.zeros(len(idx), 3, 320, 256), torch.zeros(len(idx), 2), torch.zeros(len(idx), 2)
    r = crop_from_dets(img, boxes, inps, pt1, pt2)
    assert r[0] is inps and r[1] is pt1 and r[2] is pt2
    np.testing.assert_array_equal(pt1.numpy(), e["crop_pt1"][idx])
    np.testing.assert_array_equal(pt2.numpy(), e["crop_pt2"][idx])
    assert np.abs(inps.reshape(len(idx), -1).numpy()[:, e["crop_samp_idx"]] - e["crop_samples"][idx]).max() <= 2e-6
    np.testing.assert_allclose((before - img)[:, 0, 0].numpy(), [0.406, 0.457, 0.480], atol=1e-6)   # in-place means


def test_decode_select_fused_equals_the_two_kernel_path(engines, cuda):
    """Round 4 node diet: DetectionLayer decode + write_results in one launch when nobody reads the prediction tensor
    (csrc/yolo_tail.hip, the single select from the head rows).  Bit-identical select records to decode -> select, for detections at several
    confidence thresholds and for the no-detection case (yolo/darknet.py:129-169, yolo/util.py:118-223)."""
    det, _ = engines
    x = torch.cat([helpers.yolo_input_from_frame(f) for f in helpers.frames(4)]).to(cuda)
    for conf in (0.01, 0.3, 0.5, 0.999999):
        fused = det.forward_select(x, confidence=conf)
        two, pred = det.forward_select(x, confidence=conf, want_pred=True)
        assert torch.equal(fused.view(torch.int32), two.view(torch.int32)), conf
        idx = fused[:, 0].contiguous().view(torch.int32).cpu()
        for b in range(4):
            if int(idx[b]) >= 0:
                assert float(pred[b, int(idx[b]), 4]) == float(fused[b, 5]) > conf


def test_pipeline_prepare_builds_the_graph_without_running(engines, cuda):
    """bp_pipeline_prepare (set-up step: capture + instantiate, nothing executes): results untouched until the first run, which is then
    a plain graph launch with the same record as an unprepared pipeline's."""
    det, pose = engines
    fr = helpers.frames(1)[0]
    plain = FramePipeline(det, pose, 480, 640, batch=1, use_graph=True)
    rec0 = plain.run(fr)[0].copy()
    fp = FramePipeline(det, pose, 480, 640, batch=1, use_graph=True)
    fp.prepare()
    assert float(fp.results.abs().sum()) == 0.0 and fp.kernel_count() > 100       # graph built, nothing ran
    assert np.array_equal(fp.run(fr)[0].view(np.int32), rec0.view(np.int32))
    fp.prepare()                                                                  # idempotent
    assert np.array_equal(fp.run(fr)[0].view(np.int32), rec0.view(np.int32))
