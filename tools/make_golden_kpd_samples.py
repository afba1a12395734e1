#!/usr/bin/env python3
"""Generate tests/golden/kpd_samples.npz by running the REFERENCE's own Python (build container only, like
tools/make_golden_annot.py; nothing of the reference is copied, its ``train_KPD/src/utils/{img,pose,eval}.py`` are
imported in place under stubs for the packages that are not installed).

  samples   ``generateSampleBox`` whole, on 48 x 64 frames at 20 x 16 -> 10 x 8 with 7 drawn parts: evaluation mode,
            training mode, and training mode with ``opt.addDPG``.  ``load_image`` is replaced by a function that hands
            the test frame to the reference's im_to_torch; ``random.uniform`` and ``np.random.normal`` are wrapped so that
            every draw is recorded (some are scripted, to reach every branch); ``opt.rotate = 0``, so no Rotate is built.
            ``part`` has 50 rows as the function's jointNum loop demands: the first 7 are drawn, the rest only count.
  crops     ``cropBox`` alone on seven windows at 20 x 16 and 13 x 10.
  accuracy  ``heatmapAccuracy`` and ``torch.nn.MSELoss()(out.mul(setMask), labels)`` in float32, as train() forms it.

``SpecialCrop`` and ``Pad`` of torchsample (not installed) are two stand-in classes written here: a top-left crop and
a centred constant pad, ceil before and floor after.

Conditions enforced by redrawing, with no exempt case: no window corner (first window and DPG window) within 1e-3 of an
integer, no part within 1e-3 px of a window edge, no pre-round heat-map coordinate within 1e-3 of a half-integer.

The archive is written with fixed time stamps: running this twice gives the same bytes.

Usage: python tools/make_golden_kpd_samples.py
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_shims  # noqa: E402  (only for where the reference lies)
from make_golden_annot import _stub, save_npz_fixed, stubbed  # noqa: E402

SRC = os.path.join(ref_shims.REF, "train_KPD", "src")
SEED = 31
FH, FW = 48, 64
INP, RES, KP = (20, 16), (10, 8), 7
FLIP_PAIRS = ((1, 2), (4, 7))


class SpecialCrop:
    """stand-in for torchsample.transforms.SpecialCrop(size, crop_type=1): the top-left corner"""

    def __init__(self, size, crop_type=0):
        assert crop_type == 1
        self.size = size

    def __call__(self, x):
        return x[:, :int(self.size[0]), :int(self.size[1])]


class Pad:
    """stand-in for torchsample.transforms.Pad(size): np.pad to ``size``, ceil(diff / 2) before and floor after"""

    def __init__(self, size):
        self.size = size

    def __call__(self, x):
        import torch
        x = x.numpy()
        diffs = [max(int(s) - d, 0) for d, s in zip(x.shape, self.size)]
        return torch.from_numpy(np.pad(x, [((d + 1) // 2, d // 2) for d in diffs], mode="constant"))


class Draws:
    """random.uniform / np.random.normal with every value recorded; ``unit`` scripts the U(0, 1) calls in order (None: drawn)"""

    def __init__(self, rng):
        self.rng = rng
        self.reset(())

    def reset(self, unit, replay_u=None, replay_n=None):
        self.unit, self.u, self.n = list(unit), [], []
        self.replay_u, self.replay_n = replay_u, replay_n

    def uniform(self, a, b):
        v = None
        if self.replay_u is not None:
            v = self.replay_u.pop(0)
        elif (a, b) == (0, 1) and self.unit:
            v = self.unit.pop(0)
        v = float(self.rng.uniform(a, b)) if v is None else float(v)
        self.u.append((a, b, v))
        return v

    def normal(self, mu, sd):
        v = np.float64(self.replay_n.pop(0) if self.replay_n is not None else self.rng.normal(mu, sd))
        self.n.append(float(v))
        return v


def import_reference(draws):
    sys.dont_write_bytecode = True
    opt = types.SimpleNamespace(addDPG=False, inputResH=INP[0], inputResW=INP[1], outputResH=RES[0], outputResW=RES[1], hmGauss=1,
                                rotate=0, nStack=1)
    _stub("opt", opt=opt)
    _stub("scipy.misc")
    _stub("cv2")
    ts = _stub("torchsample")
    ts.transforms = _stub("torchsample.transforms", SpecialCrop=SpecialCrop, Pad=Pad)
    pc = _stub("pycocotools")
    pc.coco = _stub("pycocotools.coco", COCO=object)
    pc.cocoeval = _stub("pycocotools.cocoeval", COCOeval=object)
    sys.path.insert(0, SRC)
    import utils.img as img
    import utils.pose as pose
    import utils.eval as ev
    pose.random = types.SimpleNamespace(uniform=draws.uniform)
    np.random.normal = draws.normal
    return opt, img, pose, ev


def heat64(part, ul, br):
    ul, br = ul.astype(np.float64), br.astype(np.float64)
    centre = (br - 1 - ul) / 2
    lenH = max(br[1] - ul[1], (br[0] - ul[0]) * INP[0] / INP[1])
    lenW = lenH * INP[1] / INP[0]
    pt = part - ul + np.maximum(0, np.array([(lenW - 1) / 2 - centre[0], (lenH - 1) / 2 - centre[1]]))
    return pt * RES[0] / lenH


def off_integer(v):
    v = np.asarray(v, dtype=np.float64)
    return bool(np.abs(v - np.rint(v)).min() > 1e-3)


def sample_ok(parts, ul, br):
    if not off_integer(np.concatenate([ul, br])):
        return False
    for p in parts:
        if p[0] <= 0:
            continue
        if np.abs(np.concatenate([p - ul.astype(np.float64), p - br.astype(np.float64)])).min() < 1e-3:
            return False
        if (p > ul).all() and (p < br).all() and np.abs(heat64(p, ul, br) - np.floor(heat64(p, ul, br)) - 0.5).min() < 1e-3:
            return False
    return True


def parse_draws(d, train, dpg, jn):
    """The recorded draws by role, following generateSampleBox's control flow."""
    u = [v for _, _, v in d.u]
    r = {"gains": np.ones(3), "patch_scale": 0.0, "patch_pos": np.zeros(2), "normal": np.zeros(4), "switch": 0.0, "flip_draw": 1.0}
    i = 0
    if train:
        r["gains"], i = np.array(u[0:3]), 3
    r["scale_rate"], i = u[i], i + 1
    if dpg:
        r["patch_scale"], i = u[i], i + 1
        if r["patch_scale"] > 0.85:
            r["patch_pos"], i = np.array(u[i:i + 2]), i + 2
        else:
            r["normal"] = np.array(d.n[0:4])
        if jn > 13 and train:
            r["switch"], i = u[i], i + 1
    if train:
        r["flip_draw"], i = u[i], i + 1
        i += 1      # the rotation's zeroing draw (opt.rotate = 0: the angle is 0 either way)
    assert i == len(u), (i, len(u))
    return r


def run_samples(rng, opt, img, pose, draws, frames):
    import torch
    pose.load_image = lambda path: img.im_to_torch(frames[int(path)].copy())
    # (mode, train, dpg, scripted U(0, 1) draws, extra counted parts, all parts outside)
    plan = [("eval", False, False, (), 0, False), ("eval no joint", False, False, (), 0, True),
            ("train flip", True, False, (0.2, None), 0, False), ("train no flip", True, False, (0.8, None), 0, False),
            ("dpg patch", True, True, (0.93, None, None, 0.3, None), 0, False),
            ("dpg normal", True, True, (0.4, 0.7, None), 0, False)]
    for sw in (0.97, 0.93, 0.89, 0.85, 0.81, 0.77, 0.73, 0.69, 0.5):
        plan.append(("dpg switch %.2f" % sw, True, True, (0.4, sw, 0.8, None), 12, False))
    plan.append(("dpg patch switch", True, True, (0.9, None, None, 0.95, 0.3, None), 12, False))
    keys = ("frame", "bndbox", "part", "train", "dpg", "gains", "scale_rate", "patch_scale", "patch_pos", "normal", "switch",
            "flip_draw", "ul0", "br0", "ul", "br", "joint_num", "inp", "out", "setMask")
    out = {k: [] for k in keys}
    names = []
    dataset = types.SimpleNamespace(flipRef=FLIP_PAIRS)
    for name, train, dpg, unit, extra, outside in plan:
        opt.addDPG = dpg
        while True:
            x1, y1 = rng.uniform(12, 24), rng.uniform(9, 16)
            box = np.array([[x1, y1, x1 + rng.uniform(16, 26), y1 + rng.uniform(14, 22)]])
            part = np.zeros((50, 2))
            lo, hi = box[0, :2], box[0, 2:]
            part[:KP] = rng.uniform(lo - 4, hi + 4, (KP, 2)) if not outside else rng.uniform(hi + 6, hi + 9, (KP, 2))
            part[1, 0] = -2.0                                   # x <= 0: never drawn
            mid = (lo + hi) / 2
            part[KP:KP + extra] = rng.uniform(mid - 1.5, mid + 1.5, (extra, 2))
            fi = int(rng.integers(0, len(frames)))
            # the windows the function forms are not returned: the same call under a spy on cropBox records them
            seen = {}
            real_crop = pose.cropBox

            def spy(im, ul, br, h, w):
                seen["ul"], seen["br"] = ul.numpy().copy(), br.numpy().copy()
                return real_crop(im, ul, br, h, w)

            pose.cropBox = spy
            draws.reset(unit)
            torch.manual_seed(0)
            inp, lab, mask = pose.generateSampleBox(str(fi), box, part, KP, "coco", (0.2, 0.3), dataset, train=train,
                                                    nJoints_coco=KP)
            pose.cropBox = real_crop
            ul, br = seen["ul"], seen["br"]
            u_keep_full = list(draws.u)
            scale = [v for a, b, v in draws.u if (a, b) == (0.2, 0.3)][0]
            tb = np.trunc(box[0]).astype(np.float32)
            w0, h0 = tb[2] - tb[0], tb[3] - tb[1]
            r32 = np.float32(scale)
            ul0 = np.array([max(0, tb[0] - w0 * r32 / 2), max(0, tb[1] - h0 * r32 / 2)], np.float32)
            br0 = np.array([min(FW - 1, tb[2] + w0 * r32 / 2), min(FH - 1, tb[3] + h0 * r32 / 2)], np.float32)
            jn = int(sum(1 for p in part if p[0] > 0 and p[0] > ul[0] and p[1] > ul[1] and p[0] < br[0] and p[1] < br[1]))
            jn_pre = jn
            n_fixed = 3 + 1 + 1 + (2 if dpg and draws.u[4][2] > 0.85 else 0)
            if dpg and len(draws.u) == n_fixed + 3:
                # the switch was drawn: jointNum (counted before the halvings, never returned) comes from the same call
                # with the same draws and a switch that halves nothing
                u_all, n_all = [v for _, _, v in draws.u], list(draws.n)
                u_all[n_fixed] = 0.5
                pose.cropBox = spy
                draws.reset((), list(u_all), list(n_all))
                pose.generateSampleBox(str(fi), box, part, KP, "coco", (0.2, 0.3), dataset, train=train, nJoints_coco=KP)
                pose.cropBox = real_crop
                jn_pre = int(sum(1 for p in part if p[0] > 0 and p[0] > seen["ul"][0] and p[1] > seen["ul"][1]
                                 and p[0] < seen["br"][0] and p[1] < seen["br"][1]))
                if not sample_ok(part, seen["ul"], seen["br"]):
                    continue
                draws.u, draws.n = u_keep_full, n_all
            if not (sample_ok(part, ul0, br0) and sample_ok(part, ul, br)):
                continue
            if name.startswith("dpg switch") and jn_pre <= 13:
                continue
            if outside and float(inp.abs().max()) != 0.0:
                continue
            break
        r = parse_draws(draws, train, dpg, jn_pre)
        vals = dict(r, frame=fi, bndbox=box[0], part=part, train=train, dpg=dpg, ul0=ul0, br0=br0, ul=ul, br=br,
                    joint_num=jn_pre, inp=inp.numpy(), out=lab.numpy(), setMask=mask.numpy())
        for k in keys:
            out[k].append(vals[k])
        names.append(name)
    return {"s_" + k: np.array(v) for k, v in out.items()}, names


CROP_WINDOWS = [("width arm, odd padding above", (5.3, 10.6), (49.2, 30.7)), ("height arm, odd padding left", (20.5, 3.2), (35.5, 44.9)),
                ("whole image", (0.0, 0.0), (64.0, 48.0)), ("right and bottom edges", (30.4, 20.2), (64.0, 48.0)),
                ("2 x 2", (10.7, 10.2), (12.9, 12.5)), ("narrow", (31.2, 4.8), (35.9, 40.1)), ("nearly square", (8.1, 6.3), (40.2, 45.9))]


def run_crops(img, frame):
    import torch
    t = img.im_to_torch(frame.copy())
    for c, m in enumerate((0.406, 0.457, 0.480)):      # generateSampleBox:26-28, restated
        t[c].add_(-m)
    out = {"c_ul": np.array([w[1] for w in CROP_WINDOWS], np.float32), "c_br": np.array([w[2] for w in CROP_WINDOWS], np.float32)}
    for res in ((20, 16), (13, 10)):
        out["c_inp_%dx%d" % res] = np.array([img.cropBox(t.clone(), torch.tensor(ul), torch.tensor(br), res[0], res[1]).numpy()
                                             for _, ul, br in CROP_WINDOWS])
    return out


def blob(hm, x, y, v=1.0):
    hm[y, x] = v
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        if 0 <= y + dy < hm.shape[0] and 0 <= x + dx < hm.shape[1]:
            hm[y + dy, x + dx] = max(hm[y + dy, x + dx], 0.5 * v)


def accuracy_cases(rng):
    cases = {}
    # a: 3 x 7 x 13 x 10 -- an undrawn label, a channel where no sample counts, a tie between two equal maxima
    out = rng.normal(0, 0.1, (3, 7, 13, 10)).astype(np.float32)
    lab = np.zeros_like(out)
    for b in range(3):
        for k in range(7):
            if k == 5 or (b, k) == (1, 2):
                continue                                        # channel 5 is empty everywhere; (1, 2) is undrawn
            x, y = int(rng.integers(1, 9)), int(rng.integers(1, 12))
            blob(lab[b, k], x, y)
            if rng.uniform() < 0.6:
                blob(out[b, k], x, y, 0.9)
    out[0, 0] = 0
    out[0, 0, 3, 7] = out[0, 0, 9, 2] = 0.75                    # tie: the lower flat index (7, 3) wins
    mask = np.ones_like(out)
    mask[2, 3] = 0                                              # a masked map: its prediction is index 0
    cases["a"] = (out, lab, mask, 13)
    # b: 2 x 3 x 80 x 64 -- squared distances of exactly 16 px^2 (on the threshold 0.5 * 80 / 10) and 17 px^2
    out = np.zeros((2, 3, 80, 64), np.float32)
    lab = np.zeros_like(out)
    for (b, k), (gx, gy), (px, py) in (((0, 0), (20, 30), (24, 30)), ((1, 0), (20, 30), (24, 31)), ((0, 1), (5, 6), (5, 6)),
                                       ((1, 1), (40, 70), (10, 3)), ((0, 2), (33, 44), (33, 40)), ((1, 2), (63, 79), (63, 79))):
        lab[b, k, gy, gx] = 1
        out[b, k, py, px] = 0.8
    out[:, :, ::7, ::5] -= np.float32(0.01)                     # (sparse, so that the archive stays small)
    cases["b"] = (out, lab, np.ones_like(out), 80)
    # c: every label empty
    out = rng.normal(0, 0.1, (2, 4, 13, 10)).astype(np.float32)
    cases["c"] = (out, np.zeros_like(out), np.ones_like(out), 13)
    return cases


def run_accuracy(opt, ev, cases):
    import torch
    res = {}
    for name, (out, lab, mask, H) in cases.items():
        opt.outputResH = H
        o, l, m = torch.from_numpy(out), torch.from_numpy(lab), torch.from_numpy(mask)
        masked = o.mul(m)
        K = out.shape[1]
        acc = ev.heatmapAccuracy(masked, l, tuple(range(1, K + 1)))
        preds, gt = ev.getPreds(masked), ev.getPreds(l)
        dists = ev.calc_dists(preds, gt, torch.ones(preds.size(0)) * H / 10)
        loss = torch.nn.MSELoss()(masked, l)
        res.update({"a_%s_out" % name: out, "a_%s_labels" % name: lab, "a_%s_mask" % name: mask, "a_%s_acc" % name: acc.numpy(),
                    "a_%s_preds" % name: preds.numpy().astype(np.int32), "a_%s_gt" % name: gt.numpy().astype(np.int32),
                    "a_%s_dists" % name: dists.numpy(), "a_%s_loss32" % name: np.float32(loss.item())})
    opt.outputResH = RES[0]
    return res


def main():
    import torch
    rng = np.random.default_rng(SEED)
    draws = Draws(rng)
    opt, img, pose, ev = import_reference(draws)
    frames = rng.integers(0, 256, (2, FH, FW, 3)).astype(np.uint8)
    frames[0, :6, :6] = 0
    frames[0, 6:12, :6] = 255
    out, names = run_samples(rng, opt, img, pose, draws, frames)
    out.update(run_crops(img, frames[1]))
    out.update(run_accuracy(opt, ev, accuracy_cases(rng)))
    meta = {
        "generator": "tools/make_golden_kpd_samples.py", "seed": SEED, "numpy": np.__version__, "torch": torch.__version__,
        "reference_ran": ["3_6Dpose_estimator/train_KPD/src/utils/pose.py: generateSampleBox",
                          "3_6Dpose_estimator/train_KPD/src/utils/img.py: im_to_torch, cropBox, transformBox, drawGaussian, flip, shuffleLR",
                          "3_6Dpose_estimator/train_KPD/src/utils/eval.py: heatmapAccuracy, getPreds, calc_dists, dist_acc"],
        "restated": ["torchsample SpecialCrop and Pad: a top-left crop and a centred constant np.pad (ceil before, floor after)",
                     "load_image: hands the test frame to im_to_torch", "generateSampleBox:26-28 (mean subtraction) in front of the cropBox-alone cases",
                     "generateSampleBox:30-41 (the first window s_ul0 / s_br0) and its jointNum loop, to record what it does not return",
                     "train(): torch.nn.MSELoss()(out.mul(setMask), labels) in float32"],
        "stubbed_third_party": sorted(set(stubbed)),
        "conditions": {"corner_integer_margin_px": 1e-3, "part_window_margin_px": 1e-3, "half_integer_margin": 1e-3, "exempt_cases": 0},
        "sample_cases": names, "crop_cases": [w[0] for w in CROP_WINDOWS], "flip_pairs": FLIP_PAIRS, "rotate": 0,
        "frame": [FH, FW], "resolution": [INP[0], INP[1], RES[0], RES[1]], "parts_drawn": KP, "part_rows": 50, "hmGauss": 1,
        "note": "one of lenH, lenW always equals the window's own size, so cropBox pads one axis at a time: the odd "
                "padding is exercised above (width arm) and to the left (height arm) in separate cases",
    }
    out.update(frames=frames, meta=np.array(json.dumps(meta, sort_keys=True)))
    path = os.path.join(ROOT, "tests", "golden", "kpd_samples.npz")
    save_npz_fixed(path, out)
    print(path, os.path.getsize(path), "bytes;", len(names), "samples")


if __name__ == "__main__":
    main()
