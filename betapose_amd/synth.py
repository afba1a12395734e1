"""Seeded synthetic inputs and weights (no LineMod data, ``.weights`` or ``.pkl``
ship with the reference -- SURVEY.md §0 F5, §8(d)).

Everything here draws from ``numpy.random.Generator(PCG64(seed))`` whose stream
is stable across numpy versions, so the same arrays are regenerated on the GPU
box, in the oracle tools and in the tests.  The distributions are chosen so
activations stay O(1) through 75 / 104 conv layers (residual branches are
damped) and the detector's objectness / the heat-map maxima are not saturated.

The second half of the module is the training-scene synthesiser: rendered, occluded and composited
frames with a sensor's depth and their ground truth, from a mesh alone (``synthesize_scenes``, ``write_scene_tree``),
and scenes of several targets with their instance masks (``instance_masks``, ``synthesize_multi``).
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from .cfg import parse_cfg_text, yolov3_single_cfg_text
from .weights import darknet_stream_layout, fastpose_modules

CAM_K = np.array([[572.4114, 0.0, 325.2611],
                  [0.0, 573.57043, 242.04899],
                  [0.0, 0.0, 1.0]])  # betapose_evaluate.py:59


def _rng(seed: int) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64(seed))


def _bn(rng, c: int, gamma_lo=0.8, gamma_hi=1.2):
    beta = rng.uniform(-0.1, 0.1, c).astype(np.float32)
    gamma = rng.uniform(gamma_lo, gamma_hi, c).astype(np.float32)
    mean = rng.uniform(-0.1, 0.1, c).astype(np.float32)
    var = rng.uniform(0.5, 1.5, c).astype(np.float32)
    return beta, gamma, mean, var


def synth_yolo_stream(seed: int = 1, blocks=None, head_gain: float = 0.25) -> np.ndarray:
    """fp32 stream (payload of a ``.weights`` file) for the YOLOv3 cfg."""
    if blocks is None:
        blocks = parse_cfg_text(yolov3_single_cfg_text())
    rng = _rng(seed)
    table = darknet_stream_layout(blocks)
    last = table[-1]
    flat = np.empty(last["weight"] + last["cout"] * last["cin"] * last["k"] ** 2, np.float32)
    for ent in table:
        co, ci, k = ent["cout"], ent["cin"], ent["k"]
        fan_in = ci * k * k
        idx = ent["index"]
        before_shortcut = idx + 1 < len(blocks) and blocks[idx + 1]["type"] == "shortcut"
        if ent["bn"]:
            lo, hi = (0.1, 0.2) if before_shortcut else (0.8, 1.2)
            beta, gamma, mean, var = _bn(rng, co, lo, hi)
            flat[ent["bn_bias"]:ent["bn_bias"] + co] = beta
            flat[ent["bn_weight"]:ent["bn_weight"] + co] = gamma
            flat[ent["bn_mean"]:ent["bn_mean"] + co] = mean
            flat[ent["bn_var"]:ent["bn_var"] + co] = var
            std = np.sqrt(2.0 / fan_in)
        else:
            # detection head: linear 1x1 conv with bias; objectness biased low so
            # that only a handful of the 10 647 candidates clear the threshold
            bias = rng.uniform(-0.5, 0.5, co).astype(np.float32)
            bias[4::6] -= 3.0
            flat[ent["bias"]:ent["bias"] + co] = bias
            std = head_gain * np.sqrt(1.0 / fan_in)
        w = rng.standard_normal(co * fan_in, dtype=np.float32) * np.float32(std)
        flat[ent["weight"]:ent["weight"] + co * fan_in] = w
    return flat


def synth_fastpose_state_dict(seed: int = 2, n_classes: int = 50,
                              out_gain: float = 1.0) -> Dict[str, np.ndarray]:
    """Random FastPose ``state_dict`` (numpy arrays, ``state_dict()`` key names)."""
    rng = _rng(seed)
    sd: Dict[str, np.ndarray] = {}
    for m in fastpose_modules(n_classes):
        n = m["name"]
        if m["kind"] == "conv":
            co, ci, k = m["cout"], m["cin"], m["k"]
            fan_in = ci * k * k
            if m["bn"]:
                damp = n.endswith(".conv3")
                lo, hi = (0.1, 0.2) if damp else (0.8, 1.2)
                beta, gamma, mean, var = _bn(rng, co, lo, hi)
                b = m["bn"]
                sd[b + ".weight"], sd[b + ".bias"] = gamma, beta
                sd[b + ".running_mean"], sd[b + ".running_var"] = mean, var
                std = np.sqrt(2.0 / fan_in)
                if n.endswith("downsample.0"):
                    std = np.sqrt(1.0 / fan_in)
            else:
                sd[n + ".bias"] = rng.uniform(0.2, 0.6, co).astype(np.float32)
                std = out_gain * np.sqrt(1.0 / fan_in)
            w = rng.standard_normal(co * fan_in, dtype=np.float32) * np.float32(std)
            sd[n + ".weight"] = w.reshape(co, ci, k, k)
        else:
            co, ci = m["cout"], m["cin"]
            w = rng.standard_normal(co * ci, dtype=np.float32) * np.float32(np.sqrt(1.0 / ci))
            sd[n + ".weight"] = w.reshape(co, ci)
            sd[n + ".bias"] = rng.uniform(-0.2, 0.2, co).astype(np.float32)
    return sd


def object_seeds(obj_id: int):
    """(detector seed, key-point-net seed) of the seeded synthetic weights of object ``obj_id``: (1, 2) for object 1
    (the fixtures' weights), distinct streams for the others so several resident objects really differ."""
    return (1, 2) if int(obj_id) == 1 else (1 + 16 * int(obj_id), 2 + 16 * int(obj_id))


def synth_frame(seed: int = 1234, h: int = 480, w: int = 640) -> np.ndarray:
    """LineMod-shaped BGR u8 frame: smooth low-res field + noise."""
    rng = _rng(seed)
    gh, gw = h // 32 + 2, w // 32 + 2
    low = rng.uniform(0, 255, (gh, gw, 3))
    ys = np.linspace(0, gh - 1.001, h)
    xs = np.linspace(0, gw - 1.001, w)
    y0 = np.floor(ys).astype(int)
    x0 = np.floor(xs).astype(int)
    fy = (ys - y0)[:, None, None]
    fx = (xs - x0)[None, :, None]
    a = low[y0][:, x0]
    b = low[y0][:, x0 + 1]
    c = low[y0 + 1][:, x0]
    d = low[y0 + 1][:, x0 + 1]
    img = (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy
    img = img + rng.normal(0, 8, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def synth_frames(n: int, seed: int = 1234) -> List[np.ndarray]:
    return [synth_frame(seed + i) for i in range(n)]


def synth_kp3d(n: int = 50, seed: int = 7, radius: float = 0.06) -> np.ndarray:
    """Non-planar 3-D key points in metres (stand-in for the designated
    key points ``assets/sifts/*.ply`` x0.001; LineMod objects are ~0.1 m)."""
    rng = _rng(seed)
    p = rng.uniform(-1, 1, (n, 3))
    return (p * np.array([radius, radius * 0.7, radius * 0.5])).astype(np.float64)


def _write_ply(path: str, pts: np.ndarray) -> None:
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "end_header\n" % len(pts))
        for x, y, z in pts:
            f.write("%.6f %.6f %.6f\n" % (x, y, z))


def _plain_yaml(v):
    """Nested dicts / lists / arrays of numbers as plain Python dicts, lists and floats (what yaml.safe_dump takes)."""
    if isinstance(v, dict):
        return {k: _plain_yaml(x) for k, x in v.items()}
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_plain_yaml(x) for x in (v.reshape(-1) if isinstance(v, np.ndarray) else v)]
    return float(v)


def write_sixd_tree(base: str, seq: int, gt_by_frame: Dict[int, list], models_mm: Dict[int, np.ndarray],
                    kpmodels_mm: Dict[int, np.ndarray], diameters_mm: Dict[int, float], cam_K=None,
                    symmetries: Dict[int, dict] = None) -> None:
    """Lay out a SIXD-format ground-truth tree the harness reads (utils/sixd.py:60-111; betapose_evaluate.py:60-75):
    ``camera.yml``, ``models/models_info.yml``, ``models/obj_XX.ply``, ``kpmodels/obj_XX.ply`` (millimetres) and
    ``test/<seq>/{gt.yml, info.yml}``.  ``gt_by_frame[nr]`` = list of ``(obj_id, R[3,3], t_mm[3], bbox[x,y,w,h])``.
    ``symmetries[obj_id]`` = ``{'symmetries_discrete': [...], 'symmetries_continuous': [...]}`` (either; the BOP fields
    metrics.symmetry_transforms reads, millimetres) is merged into that object's ``models_info.yml`` entry."""
    import os
    import yaml
    K = CAM_K if cam_K is None else np.asarray(cam_K, dtype=np.float64)
    os.makedirs(os.path.join(base, "models"), exist_ok=True)
    os.makedirs(os.path.join(base, "kpmodels"), exist_ok=True)
    sdir = os.path.join(base, "test", "%02d" % seq)
    os.makedirs(os.path.join(sdir, "rgb"), exist_ok=True)
    with open(os.path.join(base, "camera.yml"), "w") as f:
        yaml.safe_dump({"fx": float(K[0, 0]), "fy": float(K[1, 1]), "cx": float(K[0, 2]), "cy": float(K[1, 2]),
                        "depth_scale": 1.0, "width": 640, "height": 480}, f)
    with open(os.path.join(base, "models", "models_info.yml"), "w") as f:
        info = {int(k): {"diameter": float(v)} for k, v in sorted(diameters_mm.items())}
        for k, fields in sorted((symmetries or {}).items()):
            info[int(k)].update(_plain_yaml(fields))
        yaml.safe_dump(info, f)
    for oid, pts in models_mm.items():
        _write_ply(os.path.join(base, "models", "obj_%02d.ply" % oid), np.asarray(pts))
    for oid, pts in kpmodels_mm.items():
        _write_ply(os.path.join(base, "kpmodels", "obj_%02d.ply" % oid), np.asarray(pts))
    gt, info = {}, {}
    for nr, objs in sorted(gt_by_frame.items()):
        gt[int(nr)] = [{"obj_id": int(o), "cam_R_m2c": [float(v) for v in np.asarray(R).reshape(9)],
                        "cam_t_m2c": [float(v) for v in np.asarray(t).reshape(3)],
                        "obj_bb": [float(v) for v in bb]} for (o, R, t, bb) in objs]
        info[int(nr)] = {"cam_K": [float(v) for v in K.reshape(9)], "depth_scale": 1.0}
    with open(os.path.join(sdir, "gt.yml"), "w") as f:
        yaml.safe_dump(gt, f)
    with open(os.path.join(sdir, "info.yml"), "w") as f:
        yaml.safe_dump(info, f)


# ------------------------------------------------------------------------------------------------------------------------
# Training-scene synthesiser: frames, sensor depth and ground truth of a mesh, from nothing but the mesh.
# The four per-pixel stages run in libbetapose_hip (csrc/synth.hip, host twins csrc/synth_host.cpp, byte-identical); the
# geometry -- poses and occluder placement -- is numpy float64 here, and the glue draws each scene's numbers from
# generators seeded by (seed, purpose, scene number), so a scene does not depend on how the scenes are chunked.
# Frames are [I, H, W, 3] uint8 in BGR, as cv2.imread and FrameLoader give them; the files of a tree are RGB PNGs.
COMPOSE_PARAMS = 9        # csrc/synth.h SY_PARAMS: feather, r, gain[3] (Q8), offset[3], sigma (Q8)
SENSOR_PARAMS = 3         # SY_DEPTH_PARAMS: noise_k, edge_counts, hole_p
WINDOW_INTS = 6           # SY_WINDOW: bank image, x0, y0, w, h, flip
NOISE_VARIANCE = 65535    # of the noise value: 12 uniform bytes, 12 (256^2 - 1) / 12


def _images_size(size):
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise ValueError("size = (H, W) must be positive")
    return H, W


def _table(params, I, cols, name):
    t = np.ascontiguousarray(params, dtype=np.int32)
    if t.shape != (I, cols):
        raise ValueError("%s must be [%d, %d] int32" % (name, I, cols))
    return t


def compose_params(images, feather=1, blur=0, gain=(256, 256, 256), offset=(0, 0, 0), sigma=0):
    """The ``params`` table of ``compose`` with the same row for every image: [images, 9] int32.  The defaults are the
    neutral camera (the paste alone) except for the feather; ``feather=0`` makes compose equal metrics.overlay."""
    row = [int(feather), int(blur)] + [int(g) for g in gain] + [int(o) for o in offset] + [int(sigma)]
    return np.tile(np.array(row, np.int32), (int(images), 1))


def sensor_params(images, noise_k=0, edge_counts=0, hole_p=0):
    """The ``params`` table of ``sensor_depth`` with the same row for every image: [images, 3] int32."""
    return np.tile(np.array([int(noise_k), int(edge_counts), int(hole_p)], np.int32), (int(images), 1))


def procedural_background(images, size, seed, first_image=0, device=None):
    """``images`` computed backgrounds [I, H, W, 3] uint8, scenes ``first_image`` .. of ``seed``: four octaves of lattice
    value noise (cells of 64, 32, 16 and 8 pixels, bilinear in fixed point) over a base colour, the weights, the colour
    and the contrast drawn per scene.  ``device=None``: the host twin; a torch device: the kernel."""
    from . import _lib
    H, W = _images_size(size)
    I = int(images)
    if I == 0:
        return np.zeros((0, H, W, 3), np.uint8)
    side = _lib.Side(device)
    out = side.empty((I, H, W, 3), np.uint8)
    side.call("bp_synth_background", I, H, W, int(seed), int(first_image), out)
    return side.get(out)


def background_windows(bank, windows, size, device=None):
    """Backgrounds [I, H, W, 3] uint8 cut from a bank of photographs [Nb, Hb, Wb, 3] uint8: row i of ``windows``
    [I, 6] int32 = (bank image, x0, y0, w, h, flip) names a window inside its photograph, which is resampled to
    ``size`` bilinearly in fixed point with the pixel centres aligned, mirrored left to right when ``flip``."""
    from . import _lib
    H, W = _images_size(size)
    bank = np.ascontiguousarray(bank, dtype=np.uint8)
    if bank.ndim != 4 or bank.shape[3] != 3:
        raise ValueError("bank must be [Nb, Hb, Wb, 3]")
    windows = np.ascontiguousarray(windows, dtype=np.int32)
    if windows.ndim != 2 or windows.shape[1] != WINDOW_INTS:
        raise ValueError("windows must be [I, 6]: bank image, x0, y0, w, h, flip")
    I, (Nb, Hb, Wb) = len(windows), bank.shape[:3]
    if I == 0:
        return np.zeros((0, H, W, 3), np.uint8)
    side = _lib.Side(device)
    out = side.empty((I, H, W, 3), np.uint8)
    side.call("bp_synth_windows", side.put(bank), Nb, Hb, Wb, _lib.ptr(windows), I, H, W, out)
    return side.get(out)


def compose(background, color, depth, params, seed, first_image=0, device=None):
    """Training frames [I, H, W, 3] uint8: the render (``color``, ``depth`` of metrics.render_color) over ``background``
    through a camera model.  Per pixel and channel, in this order: paste with an inside feather -- where the centre has a
    fragment ``(a F + (9 - a) B + 4) // 9`` with ``a`` the pixels of the 3 x 3 neighbourhood (clamped to the image) with
    depth > 0, else B; feather off: a = 9 --, the separable binomial blur of radius r (rows, then columns, edges
    clamped, each pass rounded half up), ``((gain v + 128) >> 8) + offset``, the noise value (12 summed bytes of the
    random source minus 1530) times sigma / 2^16 rounded half up, clamp.  ``params`` [I, 9] int32 = (feather, r, gain x3
    in Q8, offset x3, sigma in Q8), see compose_params.  Image i is scene ``first_image + i`` of the random source."""
    from . import _lib
    background = np.ascontiguousarray(background, dtype=np.uint8)
    color = np.ascontiguousarray(color, dtype=np.uint8)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    if background.ndim != 4 or background.shape[3] != 3 or color.shape != background.shape or depth.shape != background.shape[:3]:
        raise ValueError("background and color must be [I, H, W, 3], depth [I, H, W]")
    I, H, W = depth.shape
    params = _table(params, I, COMPOSE_PARAMS, "params")
    if I == 0:
        return background.copy()
    side = _lib.Side(device)
    out = side.empty(background.shape, np.uint8)
    side.call("bp_synth_compose", side.put(background), side.put(color), side.put(depth), I, H, W, _lib.ptr(params), int(seed),
              int(first_image), out)
    return side.get(out)


def sensor_depth(depth, depth_scale, params, seed, first_image=0, device=None):
    """A depth sensor's image [I, H, W] uint16 of the scene depth [I, H, W] float32 (metres): counts of ``depth_scale``
    metres, rounded half up, 0 where there is nothing, at most 65 535; plus noise of sigma ``noise_k count^2 / 2^28``
    counts; a pixel whose 3 x 3 neighbourhood (clamped, background included) spans more than ``edge_counts`` counts
    becomes 0 with probability ``hole_p / 256``.  ``params`` [I, 3] int32 = (noise_k, edge_counts, hole_p)."""
    from . import _lib
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    if depth.ndim != 3:
        raise ValueError("depth must be [I, H, W]")
    I, H, W = depth.shape
    params = _table(params, I, SENSOR_PARAMS, "params")
    if I == 0:
        return np.zeros((0, H, W), np.uint16)
    side = _lib.Side(device)
    out = side.empty((I, H, W), np.uint16)
    side.call("bp_synth_sensor_depth", side.put(depth), I, H, W, float(depth_scale), _lib.ptr(params), int(seed),
              int(first_image), out)
    return side.get(out, np.uint16)


# ---- geometry on the host
_POSE_DRAWS, _OCCLUDER_DRAWS, _CAMERA_DRAWS, _WINDOW_DRAWS = 0, 1, 2, 3      # the second word of a generator's seed


def _scene_rng(seed, purpose, scene, stream=0):
    return np.random.Generator(np.random.PCG64([int(seed), int(purpose), int(scene), int(stream)]))


def _unit(v):
    return v / np.linalg.norm(v)


def _look_at(direction):
    """R0 with ``R0 @ direction = (0, 0, -1)``: the camera (x right, y down, z forward) sits along ``direction`` from the
    object and looks at it, the object's z axis pointing up in the image; at the poles its x axis takes that part."""
    z = -direction
    up = np.array([0.0, 0.0, 1.0]) if abs(direction[2]) < 0.999 else np.array([1.0, 0.0, 0.0])
    x = _unit(np.cross(z, up))
    y = np.cross(z, x)
    return np.stack([x, y, z])


def _rotation_between_z_and(ray):
    """The smallest rotation Q with ``Q @ (0, 0, 1) = ray`` (unit, z > 0)."""
    v = np.cross([0.0, 0.0, 1.0], ray)
    c = ray[2]
    V = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return np.eye(3) + V + V @ V / (1.0 + c)


def _orthonormal(R):
    """The nearest rotation: products of rotations drift by a few ulp, the renderer does not care, the contract does."""
    u, _, vt = np.linalg.svd(R)
    return u @ vt


def sample_poses(n, K, size, radius, seed, elevation=(10.0, 80.0), distance=None, inplane=(-30.0, 30.0), margin=None,
                 first_scene=0, stream=0):
    """``n`` model-to-camera poses [n, 3, 4] float64 of an object of ``radius`` round its origin.  Per scene: the
    direction from the object to the camera is uniform in area over the band ``elevation`` (degrees above the object's
    xy plane; sin(elevation) uniform, azimuth uniform), the camera looks along it with the object's z axis up and is
    rolled by an angle of ``inplane`` (degrees); the object's centre lies at ``distance`` (lo, hi; default 4 .. 8 radii)
    from the camera, on the ray of a pixel drawn uniformly at least ``margin`` pixels inside the image (default: the
    projected radius at the nearest distance, so the whole object is in view where the image allows).  Elevation and
    distance stay exactly what was drawn: the roll and the shift turn the camera about its own centre.  Scene
    ``first_scene + i`` has its own generator, seeded by (seed, scene, stream): ``stream`` selects another set of draws
    for the same scenes (synthesize_multi gives object j stream j); stream 0 is the draws this function always made."""
    H, W = _images_size(size)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    lo, hi = (4.0 * radius, 8.0 * radius) if distance is None else (float(distance[0]), float(distance[1]))
    if not radius > 0 or not lo > radius or hi < lo:
        raise ValueError("distance = (lo, hi) needs radius < lo <= hi")
    if margin is None:
        margin = min(K[0, 0], K[1, 1]) * radius / lo
    m = min(float(margin), (min(H, W) - 1) / 2.0)
    if m < 0:
        raise ValueError("margin must not be negative")
    s_lo, s_hi = np.sin(np.radians(elevation[0])), np.sin(np.radians(elevation[1]))
    poses = np.zeros((int(n), 3, 4))
    for i in range(int(n)):
        rng = _scene_rng(seed, _POSE_DRAWS, first_scene + i, stream)
        s = rng.uniform(s_lo, s_hi)
        az = rng.uniform(0.0, 2.0 * np.pi)
        roll = np.radians(rng.uniform(inplane[0], inplane[1]))
        dist = rng.uniform(lo, hi)
        u, v = rng.uniform(m, W - 1 - m), rng.uniform(m, H - 1 - m)
        c = np.sqrt(max(0.0, 1.0 - s * s))
        direction = np.array([c * np.cos(az), c * np.sin(az), s])
        ray = _unit(np.array([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], 1.0]))
        Rz = np.array([[np.cos(roll), -np.sin(roll), 0.0], [np.sin(roll), np.cos(roll), 0.0], [0.0, 0.0, 1.0]])
        poses[i, :, :3] = _orthonormal(_rotation_between_z_and(ray) @ Rz @ _look_at(direction))
        poses[i, :, 3] = dist * ray
    return poses


def place_occluders(target_poses, radii, K, size, seed, count, depth_fraction=(0.4, 0.8), lateral=1.0, first_scene=0, stream=0):
    """Poses [n, count, 3, 4] of ``count`` occluders per scene in front of the targets at ``target_poses`` [n, 3, 4]:
    a uniformly random rotation, the centre on the segment from the camera to the target's centre at a fraction of
    ``depth_fraction`` of the target's distance, moved perpendicular to that segment by up to ``lateral`` times the
    target's radius ``radii`` (uniform in area).  ``stream`` selects another set of draws for the same scenes (what
    synthesize_scenes uses for a redraw).  ``K`` and ``size`` are accepted for symmetry with sample_poses: the placement
    is along the target's ray and needs neither."""
    tp = np.asarray(target_poses, dtype=np.float64).reshape(-1, *np.shape(target_poses)[-2:])[:, :3, :4]
    radius = float(np.asarray(radii, dtype=np.float64).reshape(-1)[0])
    out = np.zeros((len(tp), int(count), 3, 4))
    for i in range(len(tp)):
        rng = _scene_rng(seed, _OCCLUDER_DRAWS, first_scene + i, stream)
        t = tp[i, :, 3]
        ray = _unit(t)
        e1 = _unit(np.cross(ray, [1.0, 0.0, 0.0] if abs(ray[0]) < 0.9 else [0.0, 1.0, 0.0]))
        e2 = np.cross(ray, e1)
        for j in range(int(count)):
            q = _unit(rng.normal(size=4))
            w, x, y, z = q
            out[i, j, :, :3] = _orthonormal(np.array(
                [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]))
            f = rng.uniform(depth_fraction[0], depth_fraction[1])
            rho, phi = lateral * radius * np.sqrt(rng.uniform(0.0, 1.0)), rng.uniform(0.0, 2.0 * np.pi)
            out[i, j, :, 3] = f * t + rho * (np.cos(phi) * e1 + np.sin(phi) * e2)
    return out


def _runs(indices):
    """Consecutive runs [a, b) of a sorted list of scene indices."""
    runs = []
    for i in indices:
        if runs and runs[-1][1] == i:
            runs[-1][1] = i + 1
        else:
            runs.append([i, i + 1])
    return runs


def _mesh3(mesh):
    """(vertices f64 [n, 3], faces int32 [F, 3], colours uint8 [n, 3] in BGR); a mesh without colours is mid grey."""
    v = np.ascontiguousarray(mesh[0], dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(mesh[1], dtype=np.int32).reshape(-1, 3)
    c = np.full((len(v), 3), 128, np.uint8) if len(mesh) < 3 or mesh[2] is None else np.ascontiguousarray(mesh[2], np.uint8)
    return v, f, c


def _mesh_texture(mesh, device):
    """render_color's texture arguments of a mesh tuple: {} for (vertices, faces[, colours]) and for a longer tuple
    without uv or texture; for (vertices, faces, colours, uv, texture) ``uv`` [F, 3, 2] and the pyramid of ``texture``
    [Ht, Wt, 3] uint8 RGB, swapped to BGR as the colours are and built ONCE, for ``device``."""
    if len(mesh) < 5 or mesh[3] is None or mesh[4] is None:
        return {}
    from . import metrics
    if isinstance(mesh[4], metrics.TextureMips):     # textured_mesh's: swapped and built already
        return dict(uv=np.ascontiguousarray(mesh[3], dtype=np.float64), texture=mesh[4])
    tex = np.asarray(mesh[4])
    if tex.dtype != np.uint8 or tex.ndim != 3 or tex.shape[2] != 3:
        raise ValueError("a mesh's texture is a uint8 image [Ht, Wt, 3] (RGB)")
    return dict(uv=np.ascontiguousarray(mesh[3], dtype=np.float64),
                texture=metrics.texture_mips(np.ascontiguousarray(tex[:, :, ::-1]), device))


def textured_mesh(mesh, device=None):
    """``mesh`` with its texture image replaced by the pyramid _mesh_texture would build from it, for ``device``: what a
    caller that synthesises chunk after chunk (synthesize.py) hands over, so that the pyramid is built once."""
    tex = _mesh_texture(mesh, device)
    return tuple(mesh) if not tex else tuple(mesh[:3]) + (tex["uv"], tex["texture"])


DEFAULT_CAMERA = dict(feather=1, blur=(0, 2), gain=(224, 288), offset=(-12, 12), sigma=(0, 768))
DEFAULT_SENSOR = dict(noise_k=512, edge_counts=30, hole_p=128)


def draw_camera(n, seed, camera=None, first_scene=0):
    """compose's table [n, 9] with each scene's blur radius, gains, offsets and sigma drawn uniformly from the integer
    ranges of ``camera`` (DEFAULT_CAMERA; a plain number fixes a value)."""
    cam = dict(DEFAULT_CAMERA, **(camera or {}))
    rng_of = lambda i: _scene_rng(seed, _CAMERA_DRAWS, first_scene + i)
    pick = lambda rng, r: int(r) if np.isscalar(r) else int(rng.integers(int(r[0]), int(r[1]) + 1))
    rows = []
    for i in range(int(n)):
        rng = rng_of(i)
        rows.append([pick(rng, cam["feather"]), pick(rng, cam["blur"])] + [pick(rng, cam["gain"]) for _ in range(3)] +
                    [pick(rng, cam["offset"]) for _ in range(3)] + [pick(rng, cam["sigma"])])
    return np.array(rows, np.int32).reshape(int(n), COMPOSE_PARAMS)


def draw_windows(n, bank_shape, size, seed, first_scene=0):
    """background_windows' table [n, 6]: per scene a photograph of the bank, the largest window of the output's aspect
    ratio scaled by a factor of 0.5 .. 1, placed uniformly, flipped with probability 1/2."""
    Nb, Hb, Wb = (int(v) for v in bank_shape[:3])
    H, W = _images_size(size)
    rows = []
    for i in range(int(n)):
        rng = _scene_rng(seed, _WINDOW_DRAWS, first_scene + i)
        k = min(Wb / W, Hb / H) * rng.uniform(0.5, 1.0)
        w, h = max(1, min(Wb, int(W * k))), max(1, min(Hb, int(H * k)))
        rows.append([int(rng.integers(Nb)), int(rng.integers(Wb - w + 1)), int(rng.integers(Hb - h + 1)), w, h, int(rng.integers(2))])
    return np.array(rows, np.int32).reshape(int(n), WINDOW_INTS)


def synthesize_scenes(target, occluders, K, size, n, seed, obj_ids=None, radius=None, elevation=(10.0, 80.0), distance=None,
                      inplane=(-30.0, 30.0), margin=None, depth_fraction=(0.4, 0.8), lateral=1.0, min_visib=0.3,
                      max_redraws=4, backgrounds=None, camera=None, sensor=None, depth_scale=0.001, first_scene=0,
                      ambient=0.5, light=(0.0, 0.0, 0.0), device=None):
    """``n`` training scenes of the mesh ``target`` = (vertices, faces[, colours RGB uint8]) in metres, partly hidden
    by one instance of each mesh of ``occluders``: a dict of arrays with one row per scene.  A mesh may also be
    (vertices, faces, colours, uv, texture) with ``uv`` [F, 3, 2] and ``texture`` [Ht, Wt, 3] uint8 RGB
    (metrics.load_ply_textured_mesh, load_texture): it is rendered textured (render_color's ``uv``, ``texture``; the
    pyramid is built once per mesh); only the frames' colours change with it --

      ``frames`` [n, H, W, 3] uint8 BGR, ``depth`` [n, H, W] uint16 (counts of ``depth_scale`` metres),
      ``obj_ids`` [1 + occluders] (the target first; default 1, 2, ...), ``poses`` [n, objects, 3, 4] and ``t_mm``
      [n, objects, 3] (the translation in millimetres: ``poses[..., 3]`` IS ``t_mm * 0.001``, what a SIXD reader
      computes from the written file), ``present`` [n, objects] bool, ``box_full`` [n, objects, 4] (xmin, xmax, ymin,
      ymax of each object rendered alone, -1 where it covers no pixel), the target's ``box_visible`` [n, 4] and
      ``visib_fract`` [n] against the sensor depth (annotate.mask_boxes), ``redraws`` [n] and ``params`` (compose's table).

    The target is rendered at sample_poses' poses, the occluders at place_occluders' ``into`` the same images, the
    backgrounds are procedural (or windows of the bank ``backgrounds`` [Nb, Hb, Wb, 3] BGR), compose and sensor_depth
    make the frames and the depth images.  A scene whose ``visib_fract`` is below ``min_visib`` has its occluders drawn
    again from the next stream, at most ``max_redraws`` times; after that it keeps none (``present`` False).  Everything
    is a function of (seed, scene number): ``first_scene`` shifts the scene numbers, so chunks concatenate to the whole.
    ``device=None``: the host twins throughout; a torch device: the kernels, with the same bytes."""
    from . import annotate as A, metrics
    H, W = _images_size(size)
    n = int(n)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    tv, tf, tc = _mesh3(target)
    occ = [_mesh3(m) for m in occluders]
    ttex, otex = _mesh_texture(target, device), [_mesh_texture(m, device) for m in occluders]
    ids = np.arange(1, 2 + len(occ)) if obj_ids is None else np.asarray(obj_ids, dtype=np.int64).reshape(-1)
    if len(ids) != 1 + len(occ):
        raise ValueError("obj_ids names the target and every occluder")
    if radius is None:
        radius = float(np.linalg.norm(tv, axis=1).max())
    sens = dict(DEFAULT_SENSOR, **(sensor or {}))
    sens_row = sensor_params(1, sens["noise_k"], sens["edge_counts"], sens["hole_p"])
    bgr = lambda c: np.ascontiguousarray(c[:, ::-1])

    def millimetres(p):                      # translations as the tree stores them; metres are derived from those
        t_mm = p[..., 3] * 1000.0
        p = p.copy()
        p[..., 3] = t_mm * 0.001
        return p, t_mm

    tposes, t_mm_t = millimetres(sample_poses(n, K, (H, W), radius, seed, elevation, distance, inplane, margin, first_scene))
    color_t, depth_t, _ = metrics.render_color(tposes, tv, tf, bgr(tc), K, (H, W), device, ambient=ambient, light=light, **ttex)
    md = metrics.render_depth(tposes, tv, tf, K, (H, W), device)[0]

    def sensed(depth, scenes):               # sensor depth of the listed scenes (sorted), run by run of scene numbers
        out = np.empty((len(scenes), H, W), np.uint16)
        at = 0
        for a, b in _runs(scenes):
            out[at:at + b - a] = sensor_depth(depth[at:at + b - a], depth_scale, np.tile(sens_row, (b - a, 1)), seed,
                                              first_scene + a, device)
            at += b - a
        return out

    def visibility(scenes, u16):
        boxes, counts = A.mask_boxes(md[scenes], K, A.scene_depth_from_u16(u16, depth_scale), device=device)
        return boxes, counts[:, 1] / np.maximum(counts[:, 0], 1)

    color, depth = color_t.copy(), depth_t.copy()
    oposes, t_mm_o = np.zeros((n, len(occ), 3, 4)), np.zeros((n, len(occ), 3))
    present = np.ones((n, 1 + len(occ)), bool)
    redraws = np.zeros(n, np.int32)
    pending = list(range(n)) if occ else []
    for attempt in range(int(max_redraws) + 1):
        if not pending:
            break
        p, t_mm = millimetres(np.concatenate([place_occluders(tposes[s:s + 1], radius, K, (H, W), seed, len(occ), depth_fraction,
                                                              lateral, first_scene + s, attempt) for s in pending]))
        c, d = color_t[pending], depth_t[pending]
        for j, (ov, of, oc) in enumerate(occ):
            c, d, _ = metrics.render_color(p[:, j], ov, of, bgr(oc), K, (H, W), device, ambient=ambient, light=light, into=(c, d),
                                           **otex[j])
        _, vf = visibility(pending, sensed(d, pending))
        keep = vf >= min_visib
        for k, s in enumerate(pending):
            if keep[k]:
                color[s], depth[s], oposes[s], t_mm_o[s] = c[k], d[k], p[k], t_mm[k]
            else:
                redraws[s] += 1
        pending = [s for k, s in enumerate(pending) if not keep[k]]
    for s in pending:                        # no placement passed: the scene keeps no occluder
        present[s, 1:] = False
    u16 = sensed(depth, list(range(n)))
    boxes, vf = visibility(list(range(n)), u16) if n else (np.zeros((0, 2, 4), np.int32), np.zeros(0))
    box_full = np.full((n, 1 + len(occ), 4), -1, np.int32)
    box_full[:, 0] = boxes[:, 0]
    for j, (ov, of, _) in enumerate(occ):
        rows = np.flatnonzero(present[:, 1 + j])
        if len(rows):
            alone = metrics.render_depth(oposes[rows, j], ov, of, K, (H, W), device)[0]
            box_full[rows, 1 + j] = A.mask_boxes(alone, K, device=device)[0][:, 0]
    if backgrounds is None:
        bg = procedural_background(n, (H, W), seed, first_scene, device)
    else:
        bank = np.asarray(backgrounds, dtype=np.uint8)
        bg = background_windows(bank, draw_windows(n, bank.shape, (H, W), seed, first_scene), (H, W), device)
    params = draw_camera(n, seed, camera, first_scene)
    frames = compose(bg, color, depth, params, seed, first_scene, device)
    return dict(frames=frames, depth=u16, obj_ids=ids, poses=np.concatenate([tposes[:, None], oposes], axis=1),
                t_mm=np.concatenate([t_mm_t[:, None], t_mm_o], axis=1), present=present, box_full=box_full,
                box_visible=boxes[:, 1].copy(), visib_fract=vf, redraws=redraws, params=params)


# ---- scenes of several targets
INSTANCE_STATS = 10       # csrc/synth.h SY_INST_STATS: px_all, px_visib, full box, visible box
MAX_INSTANCES = 32        # SY_INST_MAX
MULTI_STACK_FLOATS = 1 << 24      # synthesize_multi's bound on its stack of lone renders


def instance_masks(alone, present=None, device=None):
    """Who owns each pixel of ``I`` scenes of ``J`` objects: ``(ids [I, H, W] uint8, depth [I, H, W] float32, stats
    [I, J, 10] int32)`` from ``alone`` [J, I, H, W] float32 -- ``alone[j, i]`` is object j's depth image rendered alone in
    scene i (metrics.render_depth's, 0 where nothing was drawn; the renders stack in this order) -- and ``present``
    [I, J] (default: all).  Per pixel, among the present objects with a depth > 0 the smallest depth wins, among depths
    of exactly the same float32 bits the HIGHEST j: metrics.render_color(into=...)'s rule when the objects are drawn in
    ascending j.  ``ids`` = 1 + the winner (0: nothing), ``depth`` its depth (0).  ``stats[i, j]`` = (px_all, px_visib,
    full xmin, xmax, ymin, ymax, visible xmin, xmax, ymin, ymax): the pixels with ``alone[j, i] > 0`` and those with
    ``ids == j + 1``, boxes inclusive in get_bbox_from_mask order and -1 four times when their count is 0.  An object
    that is not present keeps its full count and box.  ``J <= 32``, ``H W <= 2^24``.  ``device=None``: the host twin; a
    torch device: csrc/synth_inst.hip, with the same bytes."""
    from . import _lib
    alone = np.ascontiguousarray(alone)
    if alone.dtype != np.float32 or alone.ndim != 4:
        raise ValueError("alone must be a float32 array [J, I, H, W]")
    J, I, H, W = alone.shape
    pres = np.ones((I, J), np.uint8) if present is None else np.ascontiguousarray(np.asarray(present) != 0, dtype=np.uint8)
    if pres.shape != (I, J):
        raise ValueError("present must be [%d, %d]" % (I, J))
    if I == 0:
        return np.zeros((0, H, W), np.uint8), np.zeros((0, H, W), np.float32), np.zeros((0, J, INSTANCE_STATS), np.int32)
    side = _lib.Side(device)
    ids, depth = side.empty((I, H, W), np.uint8), side.empty((I, H, W), np.float32)
    stats = side.empty((I, J, INSTANCE_STATS), np.int32)
    side.call("bp_synth_instances", side.put(alone), J, I, H, W, side.put(pres), ids, depth, stats)
    return side.get(ids), side.get(depth), side.get(stats)


def below_visibility(stats, min_visib):
    """synthesize_multi's removal rule on instance_masks' ``stats`` [..., 10]: True where an object covers no pixel
    or owns fewer than ``min_visib`` of the pixels it covers (float64)."""
    px_all, px_visib = stats[..., 0].astype(np.float64), stats[..., 1].astype(np.float64)
    return (stats[..., 0] == 0) | (px_visib < float(min_visib) * px_all)


def synthesize_multi(meshes, K, size, n, seed, obj_ids=None, min_visib=0.3, elevation=(10.0, 80.0), distance=None,
                     inplane=(-30.0, 30.0), backgrounds=None, camera=None, sensor=None, depth_scale=0.001, first_scene=0,
                     ambient=0.5, light=(0.0, 0.0, 0.0), device=None):
    """``n`` training scenes of the ``J`` meshes ``meshes`` = [(vertices, faces[, colours RGB uint8]), ...] in metres
    (or (vertices, faces, colours, uv, texture), as synthesize_scenes takes them),
    EVERY one of them a target: synthesize_scenes' dict with one row per scene and per-object shapes --

      ``frames`` [n, H, W, 3] uint8 BGR, ``depth`` [n, H, W] uint16, ``obj_ids`` [J] (default 1, 2, ...), ``poses``
      [n, J, 3, 4], ``t_mm`` [n, J, 3], ``present`` [n, J] bool, ``box_full``, ``box_visible`` [n, J, 4] (xmin, xmax, ymin,
      ymax; -1 when empty), ``visib_fract`` [n, J] = ``px_visib / max(px_all, 1)``, ``px_all``, ``px_visib`` [n, J],
      ``ids`` [n, H, W] uint8 (1 + the index j of the object that owns the pixel, 0 background), ``redraws`` [n] (zeros:
      nothing is drawn again here) and ``params``.

    Object j's poses are ``sample_poses(..., radius=its own, stream=j)`` through synthesize_scenes' millimetre round
    trip; each object is rendered alone (render_depth) and instance_masks says who owns each pixel.  Visibility is the
    renderer's own: an object's ``px_visib`` are the pixels it owns, out of the ``px_all`` it covers when alone.  The
    removal rule: an object with ``px_all == 0`` or ``px_visib < min_visib * px_all`` (float64) is dropped from its
    scene, all such objects in ONE round, and instance_masks runs once more with what is left.  Removing objects can only
    uncover the others -- a pixel's owner either stays or was removed -- so every survivor keeps at least the pixels, and
    so the fraction, it had: the survivors pass the rule again and one round is a fixed point.  A dropped object keeps
    its pose and ``box_full`` and has ``present`` False, ``px_visib`` 0 and ``box_visible`` -1.  Colour is
    render_color(into=...) over the present objects in ascending j, whose depth is instance_masks' bit for bit;
    backgrounds, compose and sensor_depth are synthesize_scenes'.  The scenes are processed in chunks of
    ``max(1, 2^24 // (J H W))``: the stack of lone renders never holds more than 2^24 floats (64 MB; one scene where a
    single one is larger), the bound annotate_sequence puts on its depth stack.  Everything is a function of (seed, scene
    number): chunks -- these and the caller's own, through ``first_scene`` -- concatenate to the whole.  ``device=None``:
    the host twins throughout; a torch device: the kernels, with the same bytes."""
    from . import metrics
    H, W = _images_size(size)
    n = int(n)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    ms = [_mesh3(m) for m in meshes]
    texs = [_mesh_texture(m, device) for m in meshes]
    J = len(ms)
    if not 1 <= J <= MAX_INSTANCES:
        raise ValueError("synthesize_multi takes 1 .. %d meshes" % MAX_INSTANCES)
    oids = np.arange(1, 1 + J) if obj_ids is None else np.asarray(obj_ids, dtype=np.int64).reshape(-1)
    if len(oids) != J or len(set(oids.tolist())) != J:
        raise ValueError("obj_ids names every mesh once")
    radii = [float(np.linalg.norm(v, axis=1).max()) for v, _, _ in ms]
    sens = dict(DEFAULT_SENSOR, **(sensor or {}))
    sens_row = sensor_params(1, sens["noise_k"], sens["edge_counts"], sens["hole_p"])
    bank = None if backgrounds is None else np.asarray(backgrounds, dtype=np.uint8)
    out = dict(frames=np.zeros((n, H, W, 3), np.uint8), depth=np.zeros((n, H, W), np.uint16), poses=np.zeros((n, J, 3, 4)),
               t_mm=np.zeros((n, J, 3)), present=np.zeros((n, J), bool), box_full=np.zeros((n, J, 4), np.int32),
               box_visible=np.zeros((n, J, 4), np.int32), visib_fract=np.zeros((n, J)), px_all=np.zeros((n, J), np.int32),
               px_visib=np.zeros((n, J), np.int32), ids=np.zeros((n, H, W), np.uint8), redraws=np.zeros(n, np.int32),
               params=np.zeros((n, COMPOSE_PARAMS), np.int32))
    step = max(1, MULTI_STACK_FLOATS // (J * H * W))
    for a in range(0, n, step):
        c = min(step, n - a)
        first = first_scene + a
        poses, alone = np.zeros((c, J, 3, 4)), np.zeros((J, c, H, W), np.float32)
        for j, (v, f, _) in enumerate(ms):
            p = sample_poses(c, K, (H, W), radii[j], seed, elevation, distance, inplane, None, first, stream=j)
            out["t_mm"][a:a + c, j] = p[..., 3] * 1000.0         # translations as the tree stores them; metres derive from those
            p[..., 3] = out["t_mm"][a:a + c, j] * 0.001
            poses[:, j] = p
            alone[j] = metrics.render_depth(p, v, f, K, (H, W), device)[0]
        ids, depth, stats = instance_masks(alone, None, device)
        present = ~below_visibility(stats, min_visib)
        if not present.all():
            ids, depth, stats = instance_masks(alone, present, device)
        color, zbuf = np.zeros((c, H, W, 3), np.uint8), np.zeros((c, H, W), np.float32)
        for j, (v, f, col) in enumerate(ms):
            rows = np.flatnonzero(present[:, j])
            if len(rows):
                color, zbuf, _ = metrics.render_color(poses[rows, j], v, f, np.ascontiguousarray(col[:, ::-1]), K, (H, W), device,
                                                      image_index=rows.astype(np.int32), images=c, ambient=ambient, light=light,
                                                      into=(color, zbuf), **texs[j])
        if not np.array_equal(zbuf.view(np.int32), depth.view(np.int32)):
            raise RuntimeError("the colour chain's depth differs from instance_masks': the tie rule is broken")
        if bank is None:
            bg = procedural_background(c, (H, W), seed, first, device)
        else:
            bg = background_windows(bank, draw_windows(c, bank.shape, (H, W), seed, first), (H, W), device)
        params = draw_camera(c, seed, camera, first)
        s = slice(a, a + c)
        out["frames"][s] = compose(bg, color, depth, params, seed, first, device)
        out["depth"][s] = sensor_depth(depth, depth_scale, np.tile(sens_row, (c, 1)), seed, first, device)
        out["poses"][s], out["present"][s], out["ids"][s], out["params"][s] = poses, present, ids, params
        out["px_all"][s], out["px_visib"][s] = stats[..., 0], stats[..., 1]
        out["box_full"][s], out["box_visible"][s] = stats[..., 2:6], stats[..., 6:10]
        out["visib_fract"][s] = stats[..., 1] / np.maximum(stats[..., 0], 1)
    out["obj_ids"] = oids
    return out


# ---- files
def _write_mesh_ply(path, vertices, faces, colors=None):
    """ASCII PLY with float64 coordinates written by repr (they read back to the same bits), optional uint8 RGB."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    with open(path, "w") as out:
        out.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n" % len(v))
        if colors is not None:
            out.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        out.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f))
        for i in range(len(v)):
            row = " ".join(repr(float(x)) for x in v[i])
            out.write(row + (" %d %d %d\n" % tuple(int(x) for x in colors[i]) if colors is not None else "\n"))
        for a, b, c in f:
            out.write("3 %d %d %d\n" % (a, b, c))


def write_png(path, array):
    """An [H, W, 3] uint8 RGB, [H, W] uint16 or [H, W] uint8 (greyscale) array as a PNG file (Pillow, as evaluate.py's
    --save_img)."""
    from PIL import Image
    a = np.ascontiguousarray(array)
    if not ((a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8) or (a.ndim == 2 and a.dtype in (np.uint16, np.uint8))):
        raise ValueError("write_png takes [H, W, 3] uint8, [H, W] uint16 or [H, W] uint8")
    Image.fromarray(a).save(path, format="PNG")


def write_scene_tree(base, seq, scenes, meshes, K, depth_scale=0.001, first_frame=0):
    """Write ``scenes`` (synthesize_scenes) as sequence ``seq`` of the SIXD tree ``base``, the layout sixd.load_sixd and
    annotate.py read: ``camera.yml`` (fx, fy, cx, cy, depth_scale in millimetres per count, width, height),
    ``models/models_info.yml`` (diameters, millimetres), ``models/obj_XX.ply``, ``test/SS/rgb/NNNN.png`` (RGB),
    ``test/SS/depth/NNNN.png`` (16 bit), ``test/SS/gt.yml`` -- per frame the objects present, the target first, with
    ``cam_R_m2c``, ``cam_t_m2c`` = the scenes' ``t_mm`` (millimetres; a reader's metres, t_mm * 0.001, are the scenes'
    poses bit for bit) and ``obj_bb`` = (xmin, ymin, xmax - xmin, ymax - ymin) of the full box -- and ``test/SS/info.yml``
    (cam_K, depth_scale).  ``meshes`` = {obj_id: (vertices in MILLIMETRES, faces[, colours RGB])}, the units of a SIXD
    model file; the scenes were rendered from those vertices times 0.001.  Floats are written by repr.  ``first_frame``
    > 0 appends a later chunk of scenes to the sequence's ``gt.yml`` and ``info.yml``.  This is the
    writer of synthesised trees; ``write_sixd_tree`` above stays the writer of the ground-truth fixtures.
    Scenes with ``ids`` (synthesize_multi) also get ``test/SS/mask/NNNN.png``, 8-bit greyscale with the owner's obj_id
    per pixel and 0 for the background (so the ids must be below 256), and every ``gt.yml`` row also carries
    ``obj_bb_visib`` (the visible box, as ``obj_bb``; -1 x4 stays -1, -1, 0, 0), ``visib_fract``, ``px_count_all`` and
    ``px_count_visib``; scenes without ``ids`` write exactly the files above."""
    import os
    import yaml
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    n, H, W = scenes["depth"].shape
    sdir = os.path.join(base, "test", "%02d" % int(seq))
    multi = "ids" in scenes
    if multi:
        owner = np.concatenate([[0], np.asarray(scenes["obj_ids"], dtype=np.int64)])
        if owner.min() < 0 or owner.max() > 255:
            raise ValueError("an instance mask holds obj_ids 1 .. 255")
        owner = owner.astype(np.uint8)
    for d in (os.path.join(base, "models"), os.path.join(sdir, "rgb"), os.path.join(sdir, "depth")) + \
            ((os.path.join(sdir, "mask"),) if multi else ()):
        os.makedirs(d, exist_ok=True)
    with open(os.path.join(base, "camera.yml"), "w") as f:
        yaml.safe_dump({"fx": float(K[0, 0]), "fy": float(K[1, 1]), "cx": float(K[0, 2]), "cy": float(K[1, 2]),
                        "depth_scale": float(depth_scale) * 1000.0, "width": W, "height": H}, f)
    info_models = {}
    for oid, mesh in sorted(meshes.items()):
        v = np.asarray(mesh[0], dtype=np.float64).reshape(-1, 3)
        hull = v if len(v) <= 2048 else v[np.unique(np.concatenate([v.argmin(0), v.argmax(0), np.arange(0, len(v), len(v) // 2048 + 1)]))]
        diam = float(np.sqrt(((hull[:, None] - hull[None]) ** 2).sum(-1)).max())
        info_models[int(oid)] = {"diameter": diam}
        _write_mesh_ply(os.path.join(base, "models", "obj_%02d.ply" % int(oid)), v, mesh[1], mesh[2] if len(mesh) > 2 else None)
    with open(os.path.join(base, "models", "models_info.yml"), "w") as f:
        yaml.safe_dump(info_models, f)
    gt, info = {}, {}
    if int(first_frame) > 0:                 # a later chunk of the sequence: keep the frames already listed
        with open(os.path.join(sdir, "gt.yml")) as f:
            gt = yaml.safe_load(f)
        with open(os.path.join(sdir, "info.yml")) as f:
            info = yaml.safe_load(f)
    for i in range(n):
        nr = int(first_frame) + i
        write_png(os.path.join(sdir, "rgb", "%04d.png" % nr), scenes["frames"][i][..., ::-1])
        write_png(os.path.join(sdir, "depth", "%04d.png" % nr), scenes["depth"][i])
        if multi:
            write_png(os.path.join(sdir, "mask", "%04d.png" % nr), owner[scenes["ids"][i]])
        rows = []
        for j, oid in enumerate(scenes["obj_ids"]):
            if not scenes["present"][i, j]:
                continue
            xmin, xmax, ymin, ymax = (int(v) for v in scenes["box_full"][i, j])
            rows.append({"obj_id": int(oid), "cam_R_m2c": [float(v) for v in scenes["poses"][i, j, :, :3].reshape(9)],
                         "cam_t_m2c": [float(v) for v in scenes["t_mm"][i, j]],
                         "obj_bb": [xmin, ymin, xmax - xmin, ymax - ymin]})
            if multi:
                xmin, xmax, ymin, ymax = (int(v) for v in scenes["box_visible"][i, j])
                rows[-1].update(obj_bb_visib=[xmin, ymin, xmax - xmin, ymax - ymin], visib_fract=float(scenes["visib_fract"][i, j]),
                                px_count_all=int(scenes["px_all"][i, j]), px_count_visib=int(scenes["px_visib"][i, j]))
        gt[nr] = rows
        info[nr] = {"cam_K": [float(v) for v in K.reshape(9)], "depth_scale": float(depth_scale) * 1000.0}
    with open(os.path.join(sdir, "gt.yml"), "w") as f:
        yaml.safe_dump(gt, f)
    with open(os.path.join(sdir, "info.yml"), "w") as f:
        yaml.safe_dump(info, f)


def export_training_set(tree, annotations, out, seq=None):
    """Lay the frames of sequence ``seq`` of the tree ``tree`` (default: its only sequence) out as the two training
    loaders expect, from the annotator's output ``annotations`` (annotate.write_annotations):
      ``out/kpd/%012d.png``                      every annotated frame in one folder, KPDSampleLoader's ``img_folder``;
      ``out/detector/NNNN.png`` + ``NNNN.txt``   image and Darknet label side by side, and ``out/detector/train.txt`` /
                                                 ``eval.txt``, the ``train=`` / ``valid=`` lists of YoloSampleLoader.
    Returns the two lists' paths.  Files are copied byte for byte."""
    import os
    import shutil
    test = os.path.join(tree, "test")
    if seq is None:
        seqs = sorted(d for d in os.listdir(test) if os.path.isdir(os.path.join(test, d)))
        if len(seqs) != 1:
            raise ValueError("%s holds %d sequences: name one with seq=" % (test, len(seqs)))
        seq = int(seqs[0])
    rgb = os.path.join(test, "%02d" % int(seq), "rgb")
    kpd, det = os.path.join(out, "kpd"), os.path.join(out, "detector")
    os.makedirs(kpd, exist_ok=True)
    os.makedirs(det, exist_ok=True)
    lists = {}
    for split in ("train", "eval"):
        with open(os.path.join(annotations, "%s.txt" % split)) as f:
            frames = [int(ln.strip()[:-len(".png")]) for ln in f if ln.strip()]
        paths = []
        for nr in frames:
            src = os.path.join(rgb, "%04d.png" % nr)
            shutil.copyfile(src, os.path.join(kpd, "%012d.png" % nr))
            shutil.copyfile(src, os.path.join(det, "%04d.png" % nr))
            shutil.copyfile(os.path.join(annotations, "labels", "%04d.txt" % nr), os.path.join(det, "%04d.txt" % nr))
            paths.append(os.path.join(det, "%04d.png" % nr))
        lists[split] = os.path.join(det, "%s.txt" % split)
        with open(lists[split], "w") as f:
            f.write("".join(p + "\n" for p in paths))
    return lists


def export_detector_set(tree, seq, labels_dir, out):
    """Lay the frames of sequence ``seq`` of the tree ``tree`` and the labels of every object (``labels_dir``:
    annotate.write_multi_labels) side by side as YoloSampleLoader expects, as export_training_set does for one class:
    ``out/NNNN.png`` + ``NNNN.txt``, ``out/train.txt`` / ``eval.txt`` (the images' paths), ``out/obj.names`` and
    ``out/obj.data`` whose ``train`` / ``valid`` / ``names`` / ``backup`` point into ``out``.  Returns the two lists' paths
    and the ``.data`` file's: ``{'train', 'eval', 'data'}``.  Images and labels are copied byte for byte."""
    import os
    import shutil
    from . import annotate as A
    rgb = os.path.join(tree, "test", "%02d" % int(seq), "rgb")
    os.makedirs(out, exist_ok=True)
    lists = {}
    for split in ("train", "eval"):
        with open(os.path.join(labels_dir, "%s.txt" % split)) as f:
            frames = [int(ln.strip()[:-len(".png")]) for ln in f if ln.strip()]
        paths = []
        for nr in frames:
            shutil.copyfile(os.path.join(rgb, "%04d.png" % nr), os.path.join(out, "%04d.png" % nr))
            shutil.copyfile(os.path.join(labels_dir, "labels", "%04d.txt" % nr), os.path.join(out, "%04d.txt" % nr))
            paths.append(os.path.join(out, "%04d.png" % nr))
        lists[split] = os.path.join(out, "%s.txt" % split)
        with open(lists[split], "w") as f:
            f.write("".join(p + "\n" for p in paths))
    with open(os.path.join(labels_dir, "obj.names")) as f:
        objects = [int(ln.strip()[len("obj_"):]) for ln in f if ln.strip()]
    A.write_detector_data(out, {o: c for c, o in enumerate(objects)})
    lists["data"] = os.path.join(out, "obj.data")
    return lists
