"""What the KPD training-sample tests share (test_kpd_samples_host.py, test_gpu_kpd_samples.py): the golden archive, the
window cases, a synthetic annotated folder and a grid_sample reference of the rotation."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLIP_PAIRS = ((1, 2), (4, 7))
ANGLES = (0.0, 17.3, -63.0, 80.0)       # 80 = 2 x rotate, the clip limit of the reference's rnd()


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "kpd_samples.npz"))
    out = {k: g[k] for k in g.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def window_cases(H, W):
    """(ul [7, 2], br [7, 2]) float32 on an H x W frame: the width arm of max() with an odd padding above, the height arm
    with an odd padding to the left, the whole image, one touching the right and bottom edges, a 2 x 2 window, a narrow
    and a nearly square one.  (One of lenH, lenW always equals the window's own size, so cropBox pads one axis at a
    time: ceil against floor is exercised per axis.)"""
    sx, sy = W / 64.0, H / 48.0
    ul = np.array([(5.3, 10.6), (20.5, 3.2), (0.0, 0.0), (30.4, 20.2), (10.7, 10.2), (31.2, 4.8), (8.1, 6.3)], np.float32)
    br = np.array([(49.2, 30.7), (35.5, 44.9), (64.0, 48.0), (64.0, 48.0), (12.9, 12.5), (35.9, 40.1), (40.2, 45.9)], np.float32)
    if (H, W) != (48, 64):
        ul, br = ul * np.float32([sx, sy]), br * np.float32([sx, sy])
        br[2] = br[3] = (W, H)
        br[4] = ul[4] + np.float32([2.2, 2.3])
    return np.ascontiguousarray(ul, np.float32), np.ascontiguousarray(br, np.float32)


def frames_of(H, W, n=2, seed=5):
    """n uint8 RGB frames with a block of 0 and a block of 255 in the first"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    f[0, :H // 4, :W // 4] = 0
    f[0, H // 4:H // 2, :W // 4] = 255
    return f


def rotate_reference(x, flip, angle_deg, perm=None):
    """F.grid_sample(bilinear, border, align_corners=True) of the flipped (and channel-swapped) map, float32 on the CPU:
    the independent check of augment_maps' rotation.  x [C, H, W]."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.array(x, dtype=np.float32))
    if flip:
        t = torch.flip(t, [2])
        if perm is not None:
            t = t[torch.as_tensor(np.asarray(perm, dtype=np.int64))]
    C, H, W = t.shape
    th = np.pi / 180.0 * angle_deg
    c, s = np.cos(th), np.sin(th)
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cr, cq = H / 2.0 - 0.5, W / 2.0 - 0.5
    r = c * (i - cr) - s * (j - cq) + cr
    q = s * (i - cr) + c * (j - cq) + cq
    grid = np.stack([2.0 * q / (W - 1) - 1.0, 2.0 * r / (H - 1) - 1.0], axis=-1).astype(np.float32)
    return F.grid_sample(t[None], torch.from_numpy(grid)[None], mode="bilinear", padding_mode="border", align_corners=True)[0].numpy()


def heat_batch(B, K, H, W, seed=9):
    """(out, labels, mask) float32 [B, K, H, W]: labels with one small blob per map (one map undrawn, one channel empty),
    outputs that hit some of them, a tie between two equal maxima in out[0, 0] and a mask with one zeroed map."""
    rng = np.random.default_rng(seed)
    out = rng.normal(0, 0.1, (B, K, H, W)).astype(np.float32)
    lab = np.zeros_like(out)
    for b in range(B):
        for k in range(K):
            if k == K - 2 or (b, k) == (1, 2):
                continue
            x, y = int(rng.integers(1, W - 1)), int(rng.integers(1, H - 1))
            lab[b, k, y, x] = 1.0
            lab[b, k, y, x - 1] = lab[b, k, y - 1, x] = 0.5
            if rng.uniform() < 0.6:
                out[b, k, y, x] = 0.9
    out[0, 0] = 0
    out[0, 0, 3, W - 3] = out[0, 0, H - 4, 2] = 0.75
    mask = np.ones_like(out)
    mask[B - 1, 3] = 0
    return out, lab, mask


def threshold_batch():
    """the golden's 80 x 64 case: squared distances of exactly 16 px^2 (on the threshold) and 17 px^2"""
    g = golden()
    return np.array(g["a_b_out"]), np.array(g["a_b_labels"]), np.array(g["a_b_mask"])


def write_folder(base, n=3, H=48, W=64, Kp=7, seed=11):
    """A synthetic annotated folder: n PNG frames and annot_train.npz in annotate.write_annotations' layout.  Returns the
    path of the .npz."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(base, exist_ok=True)
    names, boxes, parts = [], [], []
    for i in range(n):
        name = "%012d.png" % i
        Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(os.path.join(base, name))
        x1, y1 = rng.uniform(W * 0.2, W * 0.35), rng.uniform(H * 0.2, H * 0.3)
        box = [x1, y1, x1 + rng.uniform(W * 0.3, W * 0.4), y1 + rng.uniform(H * 0.3, H * 0.45)]
        names.append(name)
        boxes.append(box)
        parts.append(rng.uniform([box[0] - 3, box[1] - 3], [box[2] + 3, box[3] + 3], (Kp, 2)))
    path = os.path.join(base, "annot_train.npz")
    np.savez(path, bndbox=np.array(boxes).reshape(n, 1, 4), part=np.array(parts),
             imgname=np.array([[ord(c) for c in s] for s in names], dtype=np.int64))
    return path
