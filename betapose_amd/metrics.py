"""Evaluation metrics and ground-truth helpers of the harness (utils/metrics.py:10-33,77-127;
utils/model.py:29-46,79-85; utils/sixd.py:60-111), numpy f64."""
from __future__ import annotations

import os
from typing import Dict, List

import numpy as np


def add_err(gt_pose, est_pose, model):
    a = model @ gt_pose[:3, :3].T + gt_pose[:3, 3]
    b = model @ est_pose[:3, :3].T + est_pose[:3, 3]
    return float(np.mean(np.linalg.norm(a - b, axis=1)))


def projection_error_2d(gt_pose, est_pose, model, cam):
    m = np.concatenate((model, np.ones((model.shape[0], 1))), axis=1)
    g = cam @ gt_pose[:3] @ m.T
    e = cam @ est_pose[:3] @ m.T
    g, e = g / g[2], e / e[2]
    return float(np.mean(np.linalg.norm(g[:2].T - e[:2].T, axis=1)))


def add_s_err(gt_pose, est_pose, model):
    """ADD-S, the LineMod score of symmetric objects: the mean over the ground-truth model points of the distance to
    the CLOSEST estimated model point, mean_i min_j |T_g x_i - T_e x_j|.  The reference has it only as the debug loop
    it keeps commented out in add_err (utils/metrics.py:23-33), which stops after the first five ground-truth vertices
    (``if idx_A > 4: break``); that truncation is not followed here -- every vertex is a query and every vertex a
    candidate.  Brute force in the camera frame over chunks of queries so memory stays bounded (``est == gt`` gives
    exactly 0).  ``bp_pose_errors`` computes the same on the GPU, in the ground-truth object frame."""
    model = np.asarray(model, dtype=np.float64)
    gt_pose, est_pose = np.asarray(gt_pose, dtype=np.float64), np.asarray(est_pose, dtype=np.float64)
    qry = model @ gt_pose[:3, :3].T + gt_pose[:3, 3]
    cand = model @ est_pose[:3, :3].T + est_pose[:3, 3]
    n = len(model)
    step = max(1, (1 << 16) // max(n, 1))       # ~64 Ki distances (512 KB, cache-resident) per chunk
    best = np.empty(n)
    for s in range(0, n, step):
        q = qry[s:s + step]
        d = np.square(q[:, 0:1] - cand[None, :, 0])
        d += np.square(q[:, 1:2] - cand[None, :, 1])
        d += np.square(q[:, 2:3] - cand[None, :, 2])
        best[s:s + step] = d.min(axis=1)
    return float(np.mean(np.sqrt(best)))


WANT_ADD, WANT_ADDS, WANT_2D = 1, 2, 4      # bp_pose_errors' `want` bits


def pose_errors(gt_poses, est_poses, model, cam, device=None, want=WANT_ADD | WANT_ADDS | WANT_2D):
    """(ADD, ADD-S, 2-D projection error) of P pose pairs of one model as three float64 arrays [P] (metres, metres,
    pixels).  Poses are [P, 4, 4] or [P, 3, 4]; ``cam`` the 3x3 K of the 2-D error.  ``device=None``: the host numpy
    functions pair by pair; a torch device: one ``bp_pose_errors`` call on it.  ``want`` selects the columns
    (WANT_* bits); the others are NaN."""
    gt = np.asarray(gt_poses, dtype=np.float64).reshape(-1, *np.shape(gt_poses)[-2:])[:, :3, :4]
    est = np.asarray(est_poses, dtype=np.float64).reshape(-1, *np.shape(est_poses)[-2:])[:, :3, :4]
    if gt.shape != est.shape:
        raise ValueError("gt_poses and est_poses differ in shape: %s vs %s" % (gt.shape, est.shape))
    model = np.ascontiguousarray(model, dtype=np.float64).reshape(-1, 3)
    P = len(gt)
    out = np.full((P, 3), np.nan)
    if P == 0:
        return out[:, 0], out[:, 1], out[:, 2]
    if device is None:
        for p in range(P):
            g, e = np.vstack((gt[p], [0, 0, 0, 1])), np.vstack((est[p], [0, 0, 0, 1]))
            if want & WANT_ADD:
                out[p, 0] = add_err(g, e, model)
            if want & WANT_ADDS:
                out[p, 1] = add_s_err(g, e, model)
            if want & WANT_2D:
                out[p, 2] = projection_error_2d(g, e, model, cam)
        return out[:, 0], out[:, 1], out[:, 2]
    from . import _lib
    side = _lib.Side(device)
    K = np.ascontiguousarray(cam, dtype=np.float64).reshape(9) if want & WANT_2D else None
    d_out = side.put(out)
    side.call("bp_pose_errors", side.put(model), len(model), side.put(gt.reshape(P, 12)), side.put(est.reshape(P, 12)), P,
              _lib.ptr(K), int(want), d_out)
    out = side.get(d_out)
    return out[:, 0], out[:, 1], out[:, 2]


def symmetry_transforms(info_entry, max_sym_disc_step=0.01, obj_id=None):
    """The symmetry set of one object as float64 [S, 3, 4] rows [R|t] in metres, from its ``models_info.yml`` entry
    (the BOP field names, translations in the file's millimetres): ``symmetries_discrete``, a list of 16-number
    row-major 4x4 transforms, and ``symmetries_continuous``, a list of ``{axis: [3], offset: [3]}``.  D = [I] + the
    discrete entries in file order; a continuous entry becomes the N = ceil(pi / max_sym_disc_step) rotations by
    i * 2 pi / N (i = 0 .. N - 1, so the identity is one of them) about the normalised axis through ``offset``; the set
    is {c o d}, d outer and c inner, further continuous entries composed on in file order.  No field: [I].  A zero axis
    or a discrete block further than 1e-6 from orthonormal raises ValueError naming ``obj_id``."""
    entry = info_entry or {}
    who = "object %s" % obj_id if obj_id is not None else "object"
    sym = [np.eye(4)]
    for k, flat in enumerate(entry.get("symmetries_discrete") or []):
        T = np.asarray(flat, dtype=np.float64).reshape(4, 4).copy()
        if np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() > 1e-6:
            raise ValueError("%s: symmetries_discrete[%d] is not orthonormal" % (who, k))
        T[:3, 3] /= 1000.0
        T[3] = [0.0, 0.0, 0.0, 1.0]
        sym.append(T)
    for k, c in enumerate(entry.get("symmetries_continuous") or []):
        axis = np.asarray(c["axis"], dtype=np.float64).reshape(3)
        offset = np.asarray(c.get("offset", [0.0, 0.0, 0.0]), dtype=np.float64).reshape(3) / 1000.0
        norm = float(np.linalg.norm(axis))
        if not norm > 0.0:
            raise ValueError("%s: symmetries_continuous[%d] has a zero axis" % (who, k))
        a = axis / norm
        A = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        N = int(np.ceil(np.pi / max_sym_disc_step))
        turns = []
        for i in range(N):
            th = i * 2.0 * np.pi / N
            T = np.eye(4)
            T[:3, :3] = np.eye(3) + np.sin(th) * A + (1.0 - np.cos(th)) * (A @ A)     # Rodrigues
            T[:3, 3] = offset - T[:3, :3] @ offset
            turns.append(T)
        sym = [c_ @ d for d in sym for c_ in turns]
    return np.stack(sym)[:, :3, :4].copy()


def load_symmetries(base, obj_id, max_sym_disc_step=0.01):
    """``symmetry_transforms`` of object ``obj_id``'s entry in ``<base>/models/models_info.yml``."""
    import yaml
    with open(os.path.join(base, "models", "models_info.yml")) as f:
        info = yaml.safe_load(f)
    return symmetry_transforms(info[obj_id], max_sym_disc_step, obj_id=obj_id)


def load_image_width(base, default=640):
    """``width`` of ``<base>/camera.yml`` (the r = width / 640 of the MSPD thresholds), ``default`` without one."""
    import yaml
    path = os.path.join(base, "camera.yml")
    if not os.path.exists(path):
        return default
    with open(path) as f:
        return int((yaml.safe_load(f) or {}).get("width", default))


def _sym44(syms):
    s = np.asarray(syms, dtype=np.float64).reshape(-1, *np.shape(syms)[-2:])[:, :3, :4]
    out = np.tile(np.eye(4), (len(s), 1, 1))
    out[:, :3, :4] = s
    return out


def mssd_err(gt_pose, est_pose, model, syms):
    """BOP's maximum symmetry-aware surface distance, min_S max_x |E x - G S x| in metres: in the camera frame, one
    symmetry at a time.  ``syms`` [S, 3, 4] or [S, 4, 4] (symmetry_transforms).  ``bp_pose_errors_sym`` computes the
    same on the GPU with the symmetries folded into per-lane matrices."""
    model = np.asarray(model, dtype=np.float64).reshape(-1, 3)
    g, e = np.asarray(gt_pose, dtype=np.float64), np.asarray(est_pose, dtype=np.float64)
    pe = model @ e[:3, :3].T + e[:3, 3]
    best = np.inf
    for S in _sym44(syms):
        ms = model @ S[:3, :3].T + S[:3, 3]
        pg = ms @ g[:3, :3].T + g[:3, 3]
        best = min(best, float(np.linalg.norm(pe - pg, axis=1).max()))
    return best


def mspd_err(gt_pose, est_pose, model, cam, syms):
    """BOP's maximum symmetry-aware projection distance, min_S max_x |proj(E x) - proj(G S x)| in pixels, with
    proj(X) = (K X)[:2] / (K X)[2]; one symmetry at a time, as mssd_err."""
    model = np.asarray(model, dtype=np.float64).reshape(-1, 3)
    g, e = np.asarray(gt_pose, dtype=np.float64), np.asarray(est_pose, dtype=np.float64)
    cam = np.asarray(cam, dtype=np.float64)

    def proj(X):
        u = X @ cam.T
        return u[:, :2] / u[:, 2:3]
    pe = proj(model @ e[:3, :3].T + e[:3, 3])
    best = np.inf
    for S in _sym44(syms):
        ms = model @ S[:3, :3].T + S[:3, 3]
        pg = proj(ms @ g[:3, :3].T + g[:3, 3])
        best = min(best, float(np.linalg.norm(pe - pg, axis=1).max()))
    return best


WANT_MSSD, WANT_MSPD = 1, 2                 # bp_pose_errors_sym's `want` bits
BOP_MSSD_THETAS = tuple(0.05 * k for k in range(1, 11))     # fractions of the object diameter
BOP_MSPD_THETAS = tuple(5.0 * k for k in range(1, 11))      # pixels at a 640-wide image


def pose_errors_sym(gt_poses, est_poses, model, cam, syms, device=None, want=WANT_MSSD | WANT_MSPD):
    """(MSSD, MSPD) of P pose pairs of one model over its symmetry set as two float64 arrays [P] (metres, pixels).
    Poses are [P, 4, 4] or [P, 3, 4], ``syms`` [S, 3, 4] or [S, 4, 4]; ``cam`` the 3x3 K of MSPD.  ``device=None``:
    mssd_err / mspd_err pair by pair; a torch device: one ``bp_pose_errors_sym`` call on it.  ``want`` selects the
    columns (WANT_MSSD, WANT_MSPD); the others are NaN."""
    gt = np.asarray(gt_poses, dtype=np.float64).reshape(-1, *np.shape(gt_poses)[-2:])[:, :3, :4]
    est = np.asarray(est_poses, dtype=np.float64).reshape(-1, *np.shape(est_poses)[-2:])[:, :3, :4]
    if gt.shape != est.shape:
        raise ValueError("gt_poses and est_poses differ in shape: %s vs %s" % (gt.shape, est.shape))
    model = np.ascontiguousarray(model, dtype=np.float64).reshape(-1, 3)
    sym = np.ascontiguousarray(_sym44(syms)[:, :3, :4])
    if len(sym) < 1:
        raise ValueError("the symmetry set is empty (it holds at least the identity)")
    P = len(gt)
    out = np.full((P, 2), np.nan)
    if P == 0:
        return out[:, 0], out[:, 1]
    if device is None:
        for p in range(P):
            if want & WANT_MSSD:
                out[p, 0] = mssd_err(gt[p], est[p], model, sym)
            if want & WANT_MSPD:
                out[p, 1] = mspd_err(gt[p], est[p], model, cam, sym)
        return out[:, 0], out[:, 1]
    from . import _lib
    side = _lib.Side(device)
    K = np.ascontiguousarray(cam, dtype=np.float64).reshape(9) if want & WANT_MSPD else None
    d_out = side.put(out)
    side.call("bp_pose_errors_sym", side.put(model), len(model), side.put(gt.reshape(P, 12)), side.put(est.reshape(P, 12)), P,
              side.put(sym), len(sym), _lib.ptr(K), int(want), d_out)
    out = side.get(d_out)
    return out[:, 0], out[:, 1]


def rot_error(gt_pose, est_pose):
    """Angle of the relative rotation in degrees, 0..180 (utils/metrics.py:35-67 computes the same angle through
    quaternions)."""
    R = np.asarray(gt_pose)[:3, :3] @ np.asarray(est_pose)[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))


def trans_error(gt_pose, est_pose):
    """(norm, per-axis absolute) translation error (utils/metrics.py:70-74)."""
    d = np.asarray(gt_pose)[:3, 3] - np.asarray(est_pose)[:3, 3]
    return float(np.linalg.norm(d)), np.abs(d)


def iou(gt_box, est_box):
    xA, yA = max(gt_box[0], est_box[0]), max(gt_box[1], est_box[1])
    xB, yB = min(gt_box[2], est_box[2]), min(gt_box[3], est_box[3])
    if xB <= xA or yB <= yA:
        return 0.0
    inter = (xB - xA) * (yB - yA)
    A = (gt_box[2] - gt_box[0]) * (gt_box[3] - gt_box[1])
    B = (est_box[2] - est_box[0]) * (est_box[3] - est_box[1])
    return inter / float(A + B - inter)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def load_ply_vertices(path: str) -> np.ndarray:
    """Vertex x, y, z of a .ply file as float64 [n, 3] -- what ``Model3D.load`` takes from plyfile
    (utils/model.py:79-85).  ASCII and binary (little / big endian) files; the vertex element must come first, as in
    the SIXD models and the designator's key-point files."""
    with open(path, "rb") as f:
        head = b""
        while not head.rstrip().endswith(b"end_header"):
            line = f.readline()
            if not line:
                raise ValueError("%s: no end_header" % path)
            head += line
        lines = [ln.strip() for ln in head.decode("ascii", "replace").split("\n") if ln.strip()]
        if not lines or lines[0] != "ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, n, props, elem_order, cur = None, 0, [], [], None
        for ln in lines[1:]:
            tok = ln.split()
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                cur = tok[1]
                elem_order.append(cur)
                if cur == "vertex":
                    n = int(tok[2])
            elif tok[0] == "property" and cur == "vertex":
                if tok[1] == "list":
                    raise ValueError("%s: list property in the vertex element" % path)
                if tok[1] not in _PLY_TYPES:
                    raise ValueError("%s: unknown property type %s" % (path, tok[1]))
                props.append((tok[2], _PLY_TYPES[tok[1]]))
        if fmt is None or not elem_order or elem_order[0] != "vertex":
            raise ValueError("%s: the vertex element must be the first element" % path)
        names = [p_[0] for p_ in props]
        if not all(a in names for a in ("x", "y", "z")):
            raise ValueError("%s: vertex element without x, y, z" % path)
        if fmt == "ascii":
            ix = [names.index(a) for a in ("x", "y", "z")]
            rows = []
            for _ in range(n):
                tok = f.readline().split()
                if len(tok) < len(names):
                    raise ValueError("%s: truncated vertex list" % path)
                rows.append([float(tok[i]) for i in ix])
            return np.array(rows, dtype=np.float64).reshape(n, 3)
        if fmt not in ("binary_little_endian", "binary_big_endian"):
            raise ValueError("%s: unknown PLY format %s" % (path, fmt))
        end = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(nm, end + t) for nm, t in props])
        buf = f.read(n * dt.itemsize)
        if len(buf) < n * dt.itemsize:
            raise ValueError("%s: truncated vertex data" % path)
        v = np.frombuffer(buf, dtype=dt, count=n)
        return np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float64)


def load_ply_mesh(path: str):
    """``(vertices [n, 3] float64, faces [F, 3] int32)`` of a .ply file: the x, y, z of its vertex element as
    ``load_ply_vertices`` reads them (same formats, same units: the file's own, nothing is scaled) and the
    ``vertex_indices`` / ``vertex_index`` list of its face element.  A polygon of more than three vertices is
    fan-triangulated about its first vertex, (v0, v1, v2), (v0, v2, v3), ...; one of fewer than three is dropped."""
    return _read_ply_mesh(path)[0][:2]


def load_ply_colored_mesh(path: str):
    """``(vertices [n, 3] float64, faces [F, 3] int32, colors [n, 3] uint8 RGB)``: ``load_ply_mesh`` plus the ``red``,
    ``green``, ``blue`` properties of the vertex element (ASCII and both binary byte orders; float colours in [0, 1]
    are scaled to 0 .. 255).  A file without them gives 128 everywhere, the reference's 0.5 grey (utils/model.py)."""
    vertices, faces, colors = _read_ply_mesh(path)[0]
    if colors is None:
        colors = np.full((len(vertices), 3), 128, np.uint8)
    return vertices, faces, colors


def load_ply_textured_mesh(path: str):
    """``(vertices, faces, colors, uv, texture_file)``: ``load_ply_colored_mesh`` plus the mesh's texture coordinates and
    the image they refer to.  ``uv`` [F, 3, 2] float64 holds one (u, v) per face corner (v upwards: v = 1 is the image's
    top row), or is None when the file has none.  Two layouts are read, in ASCII and both binary byte orders: scalar
    vertex properties ``texture_u`` / ``texture_v`` (also ``u`` / ``v`` and ``s`` / ``t``), copied to the corners of every
    face, and a face ``property list uchar float texcoord`` of 2 k floats for a k-gon, which fan triangulation carries
    along exactly as it carries the indices (and which survives seams); where a file has both, the face list wins.
    ``texture_file`` is the path named by the first ``comment TextureFile NAME``, resolved against the PLY's folder, or
    None."""
    (vertices, faces, colors), uv, texture_file = _read_ply_mesh(path)
    if colors is None:
        colors = np.full((len(vertices), 3), 128, np.uint8)
    return vertices, faces, colors, uv, texture_file


TEXTURE_MAX_SIZE = 8192       # csrc/raster_texture_math.inc TX_MAX_SIZE


def load_texture(path: str) -> np.ndarray:
    """A PNG file as a texture [Ht, Wt, 3] uint8 RGB, row 0 the top of the image (the project's own decoder,
    frame_loader.decode_png: grey, RGB and RGBA at 8 bits; alpha is dropped)."""
    from . import frame_loader
    with open(path, "rb") as f:
        data = f.read()
    return np.ascontiguousarray(frame_loader.decode_png(data)[:, :, ::-1])


def texture_levels(Wt, Ht):
    """Levels of the full pyramid of a Wt x Ht image: 1 + ceil(log2(max(Wt, Ht)))."""
    levels, w, h = 1, int(Wt), int(Ht)
    while w > 1 or h > 1:
        w, h, levels = (w + 1) >> 1, (h + 1) >> 1, levels + 1
    return levels


class TextureMips:
    """A packed mip pyramid (``texture_mips``): ``data`` uint32 [texels] (numpy on the host, a torch tensor on a
    device), level 0 = the Wt x Ht image, one dword a texel with channel k in byte k, the levels one after the other."""

    def __init__(self, data, Wt, Ht, levels, device):
        self.data, self.Wt, self.Ht, self.levels, self.device = data, int(Wt), int(Ht), int(levels), device

    def level(self, l):
        """Level ``l`` as a uint8 array [h, w, 3] (a copy, on the host)."""
        w, h, at = self.Wt, self.Ht, 0
        for _ in range(int(l)):
            at, w, h = at + w * h, (w + 1) >> 1, (h + 1) >> 1
        d = self.data if isinstance(self.data, np.ndarray) else self.data.cpu().numpy()
        return np.ascontiguousarray(d.view(np.uint32)[at:at + w * h].view(np.uint8).reshape(h, w, 4)[:, :, :3])


def texture_mips(texture, device=None):
    """The mip pyramid of ``texture`` [Ht, Wt, 3] uint8 as render_color takes it (a ``TextureMips``): level l + 1 has
    ceil(w / 2) x ceil(h / 2) texels, each ``(a + b + c + d + 2) >> 2`` per channel of its 2 x 2 block (the partner
    index clamped where a dimension is odd), down to 1 x 1.  ``device=None``: built by the host twin,
    for the host renderer; a torch device: by bp_texture_mips, resident there.  The two hold the same bytes."""
    from . import _lib
    tex = np.ascontiguousarray(texture)
    if tex.dtype != np.uint8 or tex.ndim != 3 or tex.shape[2] != 3 or tex.shape[0] < 1 or tex.shape[1] < 1:
        raise ValueError("a texture is a uint8 array [Ht, Wt, 3]")
    Ht, Wt = tex.shape[:2]
    if Wt > TEXTURE_MAX_SIZE or Ht > TEXTURE_MAX_SIZE:
        raise ValueError("a texture must not exceed %d x %d (got %d x %d)" % (TEXTURE_MAX_SIZE, TEXTURE_MAX_SIZE, Wt, Ht))
    levels = texture_levels(Wt, Ht)
    texels = _lib.lib().bp_texture_mips_bytes(Wt, Ht, levels) // 4
    side = _lib.Side(device)
    data = side.empty(texels, np.uint32)
    side.call("bp_texture_mips", side.put(tex), Wt, Ht, levels, data)
    if side.dev is not None:
        side.torch.cuda.current_stream(side.dev).synchronize()       # the uploaded texture is released on return
    return TextureMips(data, Wt, Ht, levels, side.dev)


def _ply_colors(cols, kinds):
    """uint8 [n, 3] of three colour columns; ``kinds`` their numpy type codes (a float column holds [0, 1])."""
    out = []
    for c, k in zip(cols, kinds):
        c = np.asarray(c, dtype=np.float64)
        out.append(np.clip(np.floor(c * 255.0 + 0.5) if k[0] == "f" else c, 0, 255).astype(np.uint8))
    return np.ascontiguousarray(np.stack(out, axis=1))


_PLY_UV_NAMES = (("texture_u", "texture_v"), ("u", "v"), ("s", "t"))


def _read_ply_mesh(path: str):
    """((vertices, faces, colors or None), uv [F, 3, 2] or None, texture file or None) of a .ply file; load_ply_mesh,
    load_ply_colored_mesh and load_ply_textured_mesh."""
    with open(path, "rb") as f:
        head = b""
        while not head.rstrip().endswith(b"end_header"):
            line = f.readline()
            if not line:
                raise ValueError("%s: no end_header" % path)
            head += line
        lines = [ln.strip() for ln in head.decode("ascii", "replace").split("\n") if ln.strip()]
        if not lines or lines[0] != "ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, elems = None, []                   # elems: [name, count, [(property name, type) | (name, count type, item type)]]
        texture_file = None
        for ln in lines[1:]:
            tok = ln.split()
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "comment" and len(tok) >= 3 and tok[1] == "TextureFile" and texture_file is None:
                texture_file = os.path.join(os.path.dirname(os.path.abspath(path)), ln.split(None, 2)[2])
            elif tok[0] == "element":
                elems.append([tok[1], int(tok[2]), []])
            elif tok[0] == "property" and elems:
                types = tok[2:4] if tok[1] == "list" else tok[1:2]
                for t in types:
                    if t not in _PLY_TYPES:
                        raise ValueError("%s: unknown property type %s" % (path, t))
                elems[-1][2].append((tok[-1],) + tuple(_PLY_TYPES[t] for t in types))
        if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
            raise ValueError("%s: unknown PLY format %s" % (path, fmt))
        end = ">" if fmt == "binary_big_endian" else "<"
        vertices, faces, colors = None, None, None
        vertex_uv, corner_uv = None, None           # [n, 2] of the vertex element, [F, 3, 2] of the face element's texcoord
        rgb = ("red", "green", "blue")
        for name, count, props in elems:
            has_list = any(len(p_) == 3 for p_ in props)
            names = [p_[0] for p_ in props]
            uvn = None
            if name == "vertex":
                if has_list or not all(a in names for a in ("x", "y", "z")):
                    raise ValueError("%s: the vertex element needs scalar x, y, z" % path)
                uvn = next((pair for pair in _PLY_UV_NAMES if pair[0] in names and pair[1] in names), None)
            want, want_tc = None, None
            if name == "face":
                want = next((i for i, p_ in enumerate(props) if len(p_) == 3 and p_[0] in ("vertex_indices", "vertex_index")), None)
                if want is None:
                    raise ValueError("%s: face element without a vertex_indices list" % path)
                want_tc = next((i for i, p_ in enumerate(props) if len(p_) == 3 and p_[0] == "texcoord"), None)
            rows = []
            if fmt != "ascii" and not has_list:
                dt = np.dtype([(nm, end + t) for nm, t in props])
                buf = f.read(count * dt.itemsize)
                if len(buf) < count * dt.itemsize:
                    raise ValueError("%s: truncated %s data" % (path, name))
                if name == "vertex":
                    v = np.frombuffer(buf, dtype=dt, count=count)
                    vertices = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float64)
                    if all(a in names for a in rgb):
                        colors = _ply_colors([v[a] for a in rgb], [dict(props)[a] for a in rgb])
                    if uvn:
                        vertex_uv = np.stack([v[uvn[0]], v[uvn[1]]], axis=1).astype(np.float64)
                continue
            for _ in range(count):
                vals = []
                if fmt == "ascii":
                    tok = f.readline().split()
                    k = 0
                    for p_ in props:
                        m = 1
                        if len(p_) == 3:
                            m = int(tok[k]) if k < len(tok) else 0
                            k += 1
                        if k + m > len(tok):
                            raise ValueError("%s: truncated %s list" % (path, name))
                        vals.append([float(t) for t in tok[k:k + m]])
                        k += m
                else:
                    for p_ in props:
                        m = 1
                        if len(p_) == 3:
                            ct = np.dtype(end + p_[1])
                            raw = f.read(ct.itemsize)
                            if len(raw) < ct.itemsize:
                                raise ValueError("%s: truncated %s data" % (path, name))
                            m = int(np.frombuffer(raw, dtype=ct)[0])
                        it = np.dtype(end + p_[-1])
                        raw = f.read(m * it.itemsize)
                        if len(raw) < m * it.itemsize:
                            raise ValueError("%s: truncated %s data" % (path, name))
                        vals.append(np.frombuffer(raw, dtype=it, count=m).tolist())
                rows.append(vals)
            if name == "vertex":
                ix = [names.index(a) for a in ("x", "y", "z")]
                vertices = np.array([[r[i][0] for i in ix] for r in rows], dtype=np.float64).reshape(count, 3)
                if all(a in names for a in rgb):
                    cx = [names.index(a) for a in rgb]
                    colors = _ply_colors([[r[i][0] for r in rows] for i in cx], [props[i][1] for i in cx])
                if uvn:
                    ux, vx = names.index(uvn[0]), names.index(uvn[1])
                    vertex_uv = np.array([[r[ux][0], r[vx][0]] for r in rows], dtype=np.float64).reshape(count, 2)
            elif name == "face":
                tris, corners = [], []
                for r in rows:
                    poly = [int(i) for i in r[want]]
                    tris.extend((poly[0], poly[k], poly[k + 1]) for k in range(1, len(poly) - 1))
                    if want_tc is not None and len(poly) >= 3:
                        tc = r[want_tc]
                        if len(tc) != 2 * len(poly):
                            raise ValueError("%s: a texcoord list of %d values on a face of %d vertices" % (path, len(tc), len(poly)))
                        at = lambda k: (float(tc[2 * k]), float(tc[2 * k + 1]))
                        corners.extend((at(0), at(k), at(k + 1)) for k in range(1, len(poly) - 1))
                faces = np.array(tris, dtype=np.int32).reshape(-1, 3)
                if want_tc is not None:
                    corner_uv = np.array(corners, dtype=np.float64).reshape(-1, 3, 2)
        if vertices is None or faces is None:
            raise ValueError("%s: needs a vertex and a face element" % path)
        uv = corner_uv
        if uv is None and vertex_uv is not None:
            if len(faces) and (faces.min() < 0 or faces.max() >= len(vertex_uv)):
                raise ValueError("%s: a face index lies outside [0, %d)" % (path, len(vertex_uv)))
            uv = np.ascontiguousarray(vertex_uv[faces])
        return (vertices, faces, colors), uv, texture_file


BOP_VSD_TAUS = tuple(0.05 * k for k in range(1, 11))        # misalignment tolerances, fractions of the object diameter
BOP_VSD_THETAS = tuple(0.05 * k for k in range(1, 11))      # thresholds of correctness on the VSD error
BOP_VSD_DELTA = 0.015                                       # visibility tolerance in metres
VSD_MAX_TAUS = 16                                           # csrc/raster.h VSD_MAX_TAUS


def _poses34(poses):
    return np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, *np.shape(poses)[-2:])[:, :3, :4])


def _mesh_args(vertices, faces):
    vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    if len(vertices) < 1 or len(faces) < 1:
        raise ValueError("the mesh needs at least one vertex and one face")
    if faces.min() < 0 or faces.max() >= len(vertices):
        raise ValueError("a face index lies outside [0, %d)" % len(vertices))
    return vertices, faces


def render_depth(poses, vertices, faces, K, size, device=None, pixel_center=0.0, near=0.01):
    """Depth images of a triangle mesh at P poses: ``(depth [P, H, W] float32, skipped [P] int32)``, ``size = (H, W)``.
    ``poses`` [P, 3, 4] or [P, 4, 4] model-to-camera, ``vertices`` [n, 3] and ``faces`` [F, 3] (load_ply_mesh), ``K`` 3x3,
    all float64 in the units of the poses; the depth is the camera-space z in those units, 0 where nothing was drawn.
    The centre of pixel (x, y) lies at image coordinates (x + pixel_center, y + pixel_center): 0.0 is BOP's convention
    and the one projection_error_2d and the key points are expressed in, 0.5 the reference renderer's.  Coverage is
    exact integer arithmetic (vertices snapped to 1/256 px, top-left rule, both windings), the depth of a covered pixel
    the intersection of its ray with the triangle's plane.  There is NO near-plane clipping: a triangle
    with a vertex nearer than ``near`` (or projecting beyond +-2^14 px) is dropped whole and counted in ``skipped``.
    ``device=None``: the host renderer (bp_render_depth_host, no GPU needed); a torch device: bp_render_depth on it.
    The two images are bit-identical."""
    from . import _lib
    poses = _poses34(poses)
    vertices, faces = _mesh_args(vertices, faces)
    H, W = int(size[0]), int(size[1])
    Kf = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    P = len(poses)
    if P == 0:
        return np.zeros((0, H, W), np.float32), np.zeros(0, np.int32)
    side = _lib.Side(device)
    d_poses, mesh = side.put(poses), (side.put(vertices), len(vertices), side.put(faces), len(faces))
    depth, skipped = side.empty((P, H, W), np.float32), side.empty(P, np.int32)
    rest = (_lib.ptr(Kf), H, W, float(pixel_center), float(near), depth, skipped)
    if device is None:
        side.call("bp_render_depth", d_poses, P, *mesh, *rest)
    else:
        side.call("bp_render_depth", *mesh, d_poses, P, *rest)
    return side.get(depth), side.get(skipped)


def _image_index(image_index, images, P):
    """(int32 [P] or None, I) as the colour renderer's calls take them; the library checks the rules."""
    if image_index is None:
        return None, P if images is None else int(images)
    image_index = np.ascontiguousarray(image_index, dtype=np.int32).reshape(-1)
    if len(image_index) != P:
        raise ValueError("image_index needs one entry per pose")
    return image_index, (int(image_index.max()) + 1 if images is None and P else int(images or 0))


def render_color(poses, vertices, faces, colors, K, size, device=None, image_index=None, images=None, pixel_center=0.0,
                 near=0.01, ambient=0.5, light=(0.0, 0.0, 0.0), into=None, uv=None, texture=None, mip=True):
    """Shaded colour images of a triangle mesh with per-vertex colours: ``(color [I, H, W, 3] uint8, depth [I, H, W]
    float32, skipped [P] int32)``.  Geometry, coverage and depth are ``render_depth``'s; ``colors`` [n, 3] uint8 come
    back in the channel order they were given in.  ``image_index`` [P] (non-decreasing, values in [0, ``images``)) draws
    several poses into one image; None draws pose p into image p.  Per pixel the nearest fragment wins, among equal
    depths the lowest pose, then the lowest face; its colour is the perspective-correct mix of its vertices' colours
    times ``min(ambient + 0.5 max(L . N, 0), 1)`` with the face normal N turned towards the camera and L the unit vector
    from the surface point to ``light`` (camera space): the reference's fragment shader.  Background:
    colour 0, depth 0.  ``into=(color, depth)``: accumulate over an earlier result (of any mesh); the arrays are not
    modified, the updated copies are returned.  An earlier pixel gives way to a nearer fragment and also to one of
    EXACTLY its depth (same float32 bits): the later call wins such a tie.  ``device=None``: the host twin; a torch device: bp_render_color on it.
    The two are byte-identical.
    ``texture`` (a [Ht, Wt, 3] uint8 image, or its pyramid from ``texture_mips`` built for the same ``device``) with
    ``uv`` [F, 3, 2] (load_ply_textured_mesh) takes the place of the vertex colours, which are then not read (``colors``
    may be None): the fragment's (u, v) is the corner coordinates mixed by the same weights, the level comes from the
    footprint of one pixel step in level-0 texels (comparisons against powers of four; ``mip=False``: level 0 whatever
    the footprint), the sample is one level's bilinear mix in 8-bit fixed point with wrap mode repeat, and it is lit
    and rounded as a mixed vertex colour is.  Texels come back in the channel order given.  ``into=``
    works across textured and vertex-coloured calls in either order.  Without ``texture`` the call is what it was."""
    from . import _lib
    poses = _poses34(poses)
    vertices, faces = _mesh_args(vertices, faces)
    mips = None
    if texture is not None:
        if uv is None:
            raise ValueError("a texture needs uv [F, 3, 2]")
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        if uv.shape != (len(faces), 3, 2):
            raise ValueError("uv must have the shape [F, 3, 2] = [%d, 3, 2], got %s" % (len(faces), list(uv.shape)))
        mips = texture if isinstance(texture, TextureMips) else texture_mips(texture, device)
        on_device = not isinstance(mips.data, np.ndarray)
        if on_device != (device is not None):
            raise ValueError("the pyramid was built for %s, the call is for %s: build it with texture_mips(texture, device)" %
                             (("device %s" % mips.device) if on_device else "the host", device if device is not None else "the host"))
    elif uv is not None:
        raise ValueError("uv without a texture")
    else:
        colors = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
        if len(colors) != len(vertices):
            raise ValueError("colors needs one row per vertex")
    H, W = int(size[0]), int(size[1])
    Kf = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    lt = np.ascontiguousarray(light, dtype=np.float64).reshape(3)
    P = len(poses)
    index, I = _image_index(image_index, images, P)
    if into is not None:
        color = np.array(into[0], dtype=np.uint8, order="C")
        depth = np.array(into[1], dtype=np.float32, order="C")
        I = len(depth) if images is None else I
        if color.shape != (I, H, W, 3) or depth.shape != (I, H, W):
            raise ValueError("into=(color, depth) must have the shapes [I, H, W, 3] and [I, H, W]")
    else:
        color, depth = np.zeros((I, H, W, 3), np.uint8), np.zeros((I, H, W), np.float32)
    if P == 0:
        return color, depth, np.zeros(0, np.int32)
    side = _lib.Side(device)
    if mips is not None and device is not None:
        if mips.data.device != side.dev and not (side.dev.index is None and mips.data.device.type == side.dev.type):
            raise ValueError("the pyramid lives on %s, the call is for %s" % (mips.data.device, side.dev))
        side.dev = mips.data.device
    d_poses, mesh = side.put(poses), (side.put(vertices), len(vertices), side.put(faces), len(faces))
    if mips is None:
        name, paint = "bp_render_color", (side.put(colors),)
    else:       # (the vertex colours are not read)
        name, paint = "bp_render_color_textured", (None, side.put(uv), mips.data, mips.Wt, mips.Ht, mips.levels if mip else 1)
    d_color, d_depth, skipped = side.put(color), side.put(depth), side.empty(P, np.int32)
    rest = (_lib.ptr(index), I, _lib.ptr(Kf), H, W, float(pixel_center), float(near), float(ambient), _lib.ptr(lt),
            int(into is not None), d_color, d_depth, skipped)
    if device is None:
        side.call(name, d_poses, P, *mesh, *paint, *rest)
    else:
        side.call(name, *mesh, *paint, d_poses, P, *rest)
    return side.get(d_color), side.get(d_depth), side.get(skipped)


# Model3D._compute_bbox of the reference (utils/model.py:50-72): the corners of the axis-aligned box, x outermost, then
# z, then y, min before max; their colours; the 12 edges are csrc/raster_color_math.inc rc_box_edge
BOX_CORNER_COLORS = ((1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 1.0, 1.0),
                     (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (0.5, 0.0, 0.5), (0.0, 0.5, 0.5))


def box_corners(vertices):
    """The 8 corners [8, 3] of the axis-aligned bounding box of ``vertices`` in the reference's order."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    return np.array([[(lo, hi)[k >> 2 & 1][0], (lo, hi)[k & 1][1], (lo, hi)[k >> 1 & 1][2]] for k in range(8)])


def colors_u8(colors):
    """float colours in [0, 1] -> uint8, rounded to nearest."""
    return np.clip(np.floor(np.asarray(colors, dtype=np.float64) * 255.0 + 0.5), 0, 255).astype(np.uint8)


def draw_boxes(color, poses, corners, K, corner_colors=None, device=None, image_index=None, pixel_center=0.0, near=0.01):
    """The 12 edges of the box with object-frame ``corners`` [8, 3] (box_corners) at ``poses``, one pixel wide over
    ``color`` [I, H, W, 3] uint8, no depth test; returns the drawn copy.  ``corner_colors`` [8, 3] uint8 (default: the
    reference's, as RGB); an edge mixes its two corners' colours.  An edge crossing z = ``near`` is shortened, one wholly
    behind dropped; where edges overlap the highest (pose, edge) wins.  ``device`` as render_color; byte-identical."""
    from . import _lib
    poses = _poses34(poses)
    color = np.array(color, dtype=np.uint8, order="C")
    if color.ndim != 4 or color.shape[3] != 3:
        raise ValueError("color must be [I, H, W, 3]")
    I, H, W = color.shape[:3]
    corners = np.ascontiguousarray(corners, dtype=np.float64).reshape(8, 3)
    cc = np.ascontiguousarray(colors_u8(BOX_CORNER_COLORS) if corner_colors is None else corner_colors, dtype=np.uint8).reshape(8, 3)
    Kf = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    P = len(poses)
    if P == 0:
        return color
    index, _ = _image_index(image_index, I, P)
    side = _lib.Side(device)
    d_color = side.put(color)
    side.call("bp_draw_boxes", side.put(poses), P, side.put(corners), side.put(cc), _lib.ptr(index), I, _lib.ptr(Kf), H, W,
              float(pixel_center), float(near), d_color)
    return side.get(d_color)


def overlay(frames, color, depth, alpha=128, device=None):
    """``frames`` [I, H, W, 3] uint8 with the render (``color``, ``depth`` of render_color) blended over them where
    depth > 0: ``(alpha color + (256 - alpha) frame + 128) >> 8``; alpha 256 pastes.  ``device`` as render_color."""
    from . import _lib
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    color = np.ascontiguousarray(color, dtype=np.uint8)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    if frames.ndim != 4 or frames.shape[3] != 3 or color.shape != frames.shape or depth.shape != frames.shape[:3]:
        raise ValueError("frames and color must be [I, H, W, 3], depth [I, H, W]")
    I, H, W = depth.shape
    if I == 0:
        return frames.copy()
    side = _lib.Side(device)
    out = side.empty(frames.shape, np.uint8)
    side.call("bp_overlay", side.put(frames), side.put(color), side.put(depth), I, H, W, int(alpha), out)
    return side.get(out)


def vsd_masks(depth_test, depth_gt, depth_est, K, delta, pixel_center=0.0):
    """The per-pixel quantities of vsd_err as a dict: the distance images ``dist_test``, ``dist_gt``, ``dist_est``
    (depth z times the length of the pixel's ray ((x + c - cx) / fx, (y + c - cy) / fy, 1); 0 stays 0) and the boolean
    masks ``visib_gt``, ``visib_est``, ``inter``, ``union`` of visibility mode bop19."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    H, W = np.shape(depth_gt)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    a = (x + pixel_center - K[0, 2]) / K[0, 0]
    b = (y + pixel_center - K[1, 2]) / K[1, 1]
    ray = np.sqrt(a * a + b * b + 1.0)
    dt = np.asarray(depth_test, dtype=np.float64) * ray
    dg = np.asarray(depth_gt, dtype=np.float64) * ray
    de = np.asarray(depth_est, dtype=np.float64) * ray
    vg = (dg > 0) & ((dg - dt <= delta) | (dt == 0))
    ve = ((de > 0) & ((de - dt <= delta) | (dt == 0))) | (vg & (de > 0))
    return {"dist_test": dt, "dist_gt": dg, "dist_est": de, "visib_gt": vg, "visib_est": ve, "inter": vg & ve,
            "union": vg | ve}


def vsd_err(depth_test, depth_gt, depth_est, K, delta, taus, diameter, pixel_center=0.0):
    """BOP's Visible Surface Discrepancy of one pose pair from three depth images [H, W] in one unit -- the test image
    and the renders of the ground-truth and the estimated pose, 0 = nothing / missing -- as float64 [len(taus)]: the
    toolkit's ``vsd`` with ``cost_type='step'``, ``normalized_by_diameter=True`` and visibility mode ``bop19``.
    Depths become distances from the camera centre (vsd_masks); the ground truth is visible where it is rendered and
    not more than ``delta`` behind the test surface (or the test depth is missing); the estimate likewise, and also
    wherever the ground truth is visible and the estimate is rendered.  With inter / union the pixel counts of the two
    masks' intersection and union, e(tau) = (#{p in inter: |dist_gt - dist_est| / diameter >= tau} + union - inter)
    / union, and 1.0 when the union is empty.
    This restates the published description of the metric; the BOP toolkit itself was not available to check against.
    ``bp_vsd_errors`` computes the same on the GPU from renders it makes itself."""
    m = vsd_masks(depth_test, depth_gt, depth_est, K, delta, pixel_center)
    inter, union = int(m["inter"].sum()), int(m["union"].sum())
    out = np.ones(len(taus), dtype=np.float64)
    if union == 0:
        return out
    rel = np.abs(m["dist_gt"] - m["dist_est"])[m["inter"]] / diameter
    for k, tau in enumerate(taus):
        out[k] = (int((rel >= tau).sum()) + (union - inter)) / union
    return out


def pose_errors_vsd(gt_poses, est_poses, vertices, faces, K, depth_test_u16, test_index, diameter, depth_scale=0.001,
                    delta=BOP_VSD_DELTA, taus=BOP_VSD_TAUS, device=None, chunk=0, pixel_center=0.0, near=0.01):
    """VSD of P pose pairs of one mesh: ``(err [P, n_tau] float64, counts [P, 4] int32)``.  Both poses of a pair are
    rendered (render_depth) and compared with test image ``test_index[p]`` of ``depth_test_u16`` [T, H, W] uint16,
    whose depth is ``raw * depth_scale`` in the units of the poses (0.001 for LineMod's millimetre PNGs with poses in
    metres; 0 = missing).  ``counts[p]`` = (rendered ground-truth pixels, visible ground-truth pixels, intersection,
    union), so ``counts[:, 1] / counts[:, 0]`` is BOP's visible fraction (``visib_fract``) of each annotation.
    ``device=None``: host renders and vsd_err pair by pair; a torch device: one bp_vsd_errors call on it, ``chunk``
    pairs at a time (0: a default that keeps the workspace under 256 MB).  The device results are bit-identical from
    call to call and across chunk sizes, and equal the host's."""
    gt, est = _poses34(gt_poses), _poses34(est_poses)
    if gt.shape != est.shape:
        raise ValueError("gt_poses and est_poses differ in shape: %s vs %s" % (gt.shape, est.shape))
    vertices, faces = _mesh_args(vertices, faces)
    dtest = np.ascontiguousarray(depth_test_u16)
    if dtest.dtype != np.uint16 or dtest.ndim != 3:
        raise ValueError("depth_test_u16 must be a uint16 array [T, H, W]")
    T, H, W = dtest.shape
    idx = np.ascontiguousarray(test_index, dtype=np.int32).reshape(-1)
    taus = np.ascontiguousarray(taus, dtype=np.float64).reshape(-1)
    P = len(gt)
    if len(idx) != P:
        raise ValueError("test_index needs one entry per pose pair")
    if P and (idx.min() < 0 or idx.max() >= T):
        raise ValueError("a test index lies outside [0, %d)" % T)
    if not 1 <= len(taus) <= VSD_MAX_TAUS:
        raise ValueError("between 1 and %d taus" % VSD_MAX_TAUS)
    err, counts = np.ones((P, len(taus)), np.float64), np.zeros((P, 4), np.int32)
    if P == 0:
        return err, counts
    if device is None:
        step = max(1, (1 << 24) // (H * W))
        for s in range(0, P, step):
            dg = render_depth(gt[s:s + step], vertices, faces, K, (H, W), None, pixel_center, near)[0]
            de = render_depth(est[s:s + step], vertices, faces, K, (H, W), None, pixel_center, near)[0]
            for j in range(len(dg)):
                p = s + j
                test = dtest[idx[p]].astype(np.float64) * depth_scale
                err[p] = vsd_err(test, dg[j], de[j], K, delta, taus, diameter, pixel_center)
                m = vsd_masks(test, dg[j], de[j], K, delta, pixel_center)
                counts[p] = (int((dg[j] > 0).sum()), int(m["visib_gt"].sum()), int(m["inter"].sum()), int(m["union"].sum()))
        return err, counts
    from . import _lib
    side = _lib.Side(device)
    Kf = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    d_err, d_counts = side.empty((P, len(taus)), np.float64), side.empty((P, 4), np.int32)
    side.call("bp_vsd_errors", side.put(vertices), len(vertices), side.put(faces), len(faces), side.put(gt), side.put(est), P,
              _lib.ptr(Kf), side.put(dtest), T, H, W, float(depth_scale), side.put(idx), float(delta), _lib.ptr(taus), len(taus),
              float(diameter), float(pixel_center), float(near), int(chunk), d_err, d_counts)
    return side.get(d_err), side.get(d_counts)


# ---- pose verification by gradient agreement (csrc/verify.hip, verify_host.cpp)
VERIFY_SCENE_MIN_SQ = 25             # the reference's `mags < 5` on an 8-bit image: masked iff gx^2 + gy^2 <= 24
VERIFY_RENDER_MIN_SQ = 1624975       # ... on a render that is float in [0, 1]: masked iff m2 < (4.999 * 255)^2 = 1624974.8
VERIFY_STACK_BYTES = 256 << 20       # what verify_poses keeps a chunk's render stack (colour and depth) under


def _verify_images(images, what):
    images = np.ascontiguousarray(images)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
        raise ValueError("%s must be a uint8 array [N, H, W, 3]" % what)
    if images.shape[1] < 3 or images.shape[2] < 3:
        raise ValueError("%s: H and W must be at least 3" % what)
    return images if images.flags.writeable else images.copy()          # (torch.from_numpy wants a writable array)


def _red(red_channel):
    if red_channel not in (0, 2):
        raise ValueError("red_channel must be 0 or 2")
    return int(red_channel)


def image_gradients(images, red_channel=0, min_sq=VERIFY_SCENE_MIN_SQ, device=None):
    """Unit Sobel gradients of ``images`` [I, H, W, 3] uint8: ``(grads [I, H, W, 2] float32, mags [I, H, W] float32)``,
    the reference's ``compute_grads_and_mags`` (utils/utils.py:576-585) for a stack of images.  Gray is
    ``(4899 R + 9617 G + 1868 B + 8192) >> 14`` with byte ``red_channel`` (0 or 2) as R; the Sobel is ``ksize=5`` with a
    reflect-101 border; a pixel is kept iff ``gx^2 + gy^2 >= min_sq`` (integers), its magnitude is
    ``sqrt(gx^2 + gy^2) + 0.001`` and its gradient (gx, gy) over that; a masked pixel is all 0.
    ``device=None``: the host twin; a torch device: bp_image_gradients on it.  The two are byte-identical."""
    from . import _lib
    images = _verify_images(images, "images")
    I, H, W = images.shape[:3]
    red = _red(red_channel)
    side = _lib.Side(device)
    grads, mags = side.zeros((I, H, W, 2), np.float32), side.zeros((I, H, W), np.float32)
    side.call("bp_image_gradients", side.put(images), I, H, W, red, int(min_sq), grads, mags)
    return side.get(grads), side.get(mags)


def gradient_scores(renders, frames_or_grads, frame_index, red_channel=0, render_min_sq=VERIFY_RENDER_MIN_SQ,
                    scene_min_sq=VERIFY_SCENE_MIN_SQ, device=None):
    """The verification score of P renders: ``(scores [P] float64, sums [P] uint64, counts [P] int32)``.  ``renders``
    [P, H, W, 3] uint8 (render_color's images); ``frames_or_grads`` either the frames [T, H, W, 3] uint8, whose gradients
    are taken first (image_gradients, ``scene_min_sq``), or those gradients [T, H, W, 2] float32; render p is compared
    with frame ``frame_index[p]``.  Over the render's kept pixels (``render_min_sq``) ``sums`` adds
    ``lrint(|g_render . g_scene| 2^24)`` of the unit gradients, ``counts`` is their number and ``scores = sums / 2^24 /
    (counts + 1)``: the reference's ``dot / (sum + 1)`` (utils/utils.py:602-604).  A frame index outside [0, T) gives
    score NaN, sum 0 and count -1.  ``device`` as image_gradients; the integer sum makes host and device byte-identical
    and the device's result the same from run to run."""
    from . import _lib
    renders = _verify_images(renders, "renders")
    P, H, W = renders.shape[:3]
    red = _red(red_channel)
    idx = np.ascontiguousarray(frame_index, dtype=np.int32).reshape(-1)
    if len(idx) != P:
        raise ValueError("frame_index needs one entry per render")
    scene = np.ascontiguousarray(frames_or_grads)
    is_frames = scene.dtype == np.uint8
    if is_frames:
        scene = _verify_images(scene, "frames")
    elif scene.dtype != np.float32 or scene.ndim != 4 or scene.shape[3] != 2:
        raise ValueError("frames_or_grads must be uint8 [T, H, W, 3] or float32 [T, H, W, 2]")
    if scene.shape[1:3] != (H, W):
        raise ValueError("renders are %d x %d, the frames %d x %d" % (H, W, scene.shape[1], scene.shape[2]))
    T = len(scene)
    if T < 1:
        raise ValueError("at least one frame")
    scores, sums, counts = np.zeros(P, np.float64), np.zeros(P, np.uint64), np.zeros(P, np.int32)
    if P == 0:
        return scores, sums, counts
    side = _lib.Side(device)
    d_grads = _scene_grads(side, scene, is_frames, red, scene_min_sq)
    d_scores, d_sums, d_counts = side.put(scores), side.put(sums), side.put(counts)
    side.call("bp_gradient_scores", side.put(renders), d_grads, side.put(idx), P, T, H, W, red, int(render_min_sq), d_sums,
              d_counts, d_scores)
    return side.get(d_scores), side.get(d_sums, np.uint64), side.get(d_counts)


def _scene_grads(side, scene, is_frames, red, scene_min_sq):
    """The scene's gradients [T, H, W, 2] as a buffer of ``side``: taken from the frames there, or the given ones put there."""
    if not is_frames:
        return side.put(scene)
    T, H, W = scene.shape[:3]
    grads = side.zeros((T, H, W, 2), np.float32)
    side.call("bp_image_gradients", side.put(scene), T, H, W, red, int(scene_min_sq), grads, None)
    return grads


def verify_chunk(H, W, P, chunk=0):
    """Poses per pass of verify_poses: ``chunk``, or for 0 as many as keep the render stack (3 bytes of colour and 4 of
    depth per pixel) under 256 MB; at least 1, at most P (bp_vsd_errors' convention)."""
    return max(1, min(int(chunk) if chunk else VERIFY_STACK_BYTES // (H * W * 7), max(P, 1)))


def verify_poses(poses, vertices, faces, colors, K, frames, frame_index, device=None, pixel_center=0.0, near=0.01,
                 ambient=0.5, light=(0.0, 0.0, 0.0), uv=None, texture=None, chunk=0, red_channel=0,
                 render_min_sq=VERIFY_RENDER_MIN_SQ, scene_min_sq=VERIFY_SCENE_MIN_SQ):
    """Scores P pose hypotheses of one mesh against the frames they belong to: ``(scores [P] float64, sums [P] uint64,
    counts [P] int32, skipped [P] int32)``.  Every pose is rendered into an image of its own (render_color with
    ``colors``, or with ``uv`` and ``texture`` textured; ``pixel_center``, ``near``, ``ambient``, ``light`` are its) and
    scored against frame ``frame_index[p]`` of ``frames`` [T, H, W, 3] uint8 as gradient_scores does; the highest score
    is the pose whose rendered edges agree best with the frame's (the reference's verify_6D_poses).  The colours, the
    texture and the frames share one channel order; ``red_channel`` says which byte is red.  ``chunk`` poses are
    rendered and scored at a time (verify_chunk); the results do not depend on it.  ``device=None``: the host twins; a
    torch device: frames, mesh and poses are uploaded once, each chunk is rendered (bp_render_color[_textured]) and
    scored (bp_gradient_scores) on it, and only the four result rows come back.  Byte-identical either way."""
    from . import _lib
    poses = _poses34(poses)
    vertices, faces = _mesh_args(vertices, faces)
    frames = _verify_images(frames, "frames")
    T, H, W = frames.shape[:3]
    red = _red(red_channel)
    P = len(poses)
    idx = np.ascontiguousarray(frame_index, dtype=np.int32).reshape(-1)
    if len(idx) != P:
        raise ValueError("frame_index needs one entry per pose")
    if T < 1:
        raise ValueError("at least one frame")
    if (uv is None) != (texture is None):
        raise ValueError("uv and texture are given together")
    scores, sums, counts = np.zeros(P, np.float64), np.zeros(P, np.uint64), np.zeros(P, np.int32)
    skipped = np.zeros(P, np.int32)
    if P == 0:
        return scores, sums, counts, skipped
    step = verify_chunk(H, W, P, chunk)
    if device is None:
        grads = image_gradients(frames, red, scene_min_sq)[0]
        for s in range(0, P, step):
            color, _, skipped[s:s + step] = render_color(poses[s:s + step], vertices, faces, colors, K, (H, W), None,
                                                         pixel_center=pixel_center, near=near, ambient=ambient, light=light,
                                                         uv=uv, texture=texture)
            scores[s:s + step], sums[s:s + step], counts[s:s + step] = gradient_scores(
                color, grads, idx[s:s + step], red, render_min_sq)
        return scores, sums, counts, skipped
    side = _lib.Side(device)
    Kf = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    lt = np.ascontiguousarray(light, dtype=np.float64).reshape(3)
    if texture is not None:
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        if uv.shape != (len(faces), 3, 2):
            raise ValueError("uv must have the shape [F, 3, 2] = [%d, 3, 2], got %s" % (len(faces), list(uv.shape)))
        mips = texture if isinstance(texture, TextureMips) else texture_mips(texture, side.dev)
        if isinstance(mips.data, np.ndarray):
            raise ValueError("the pyramid was built for the host, the call is for %s" % (side.dev,))
        side.dev = mips.data.device
        name, paint = "bp_render_color_textured", (None, side.put(uv), mips.data, mips.Wt, mips.Ht, mips.levels)
    else:
        colors = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
        if len(colors) != len(vertices):
            raise ValueError("colors needs one row per vertex")
        name, paint = "bp_render_color", (side.put(colors),)
    d_grads = _scene_grads(side, frames, True, red, scene_min_sq)
    mesh = (side.put(vertices), len(vertices), side.put(faces), len(faces))
    d_poses, d_idx = side.put(poses.reshape(P, 12)), side.put(idx)
    d_color, d_depth = side.empty((step, H, W, 3), np.uint8), side.empty((step, H, W), np.float32)
    d_sums, d_counts = side.empty(P, np.uint64), side.empty(P, np.int32)
    d_scores, d_skipped = side.empty(P, np.float64), side.empty(P, np.int32)
    for s in range(0, P, step):
        n = min(step, P - s)
        d_color[:n].zero_()
        d_depth[:n].zero_()
        side.call(name, *mesh, *paint, d_poses[s:s + n], n, None, n, _lib.ptr(Kf), H, W, float(pixel_center), float(near),
                  float(ambient), _lib.ptr(lt), 0, d_color, d_depth, d_skipped[s:s + n])
        side.call("bp_gradient_scores", d_color, d_grads, d_idx[s:s + n], n, T, H, W, red, int(render_min_sq), d_sums[s:s + n],
                  d_counts[s:s + n], d_scores[s:s + n])
    return side.get(d_scores), side.get(d_sums, np.uint64), side.get(d_counts), side.get(d_skipped)


ICP_ACC = 29                                                # csrc/icp.h ICP_ACC
ICP_STATUS = ("OK", "TOO_FEW", "SINGULAR", "DIVERGED", "REJECTED", "NO_IMAGE")   # stats[:, 5] (csrc/icp_math.inc)


def _icp_args(poses, vertices, faces, K, depth_test_u16, test_index):
    poses = _poses34(poses)
    vertices, faces = _mesh_args(vertices, faces)
    dtest = np.ascontiguousarray(depth_test_u16)
    if dtest.dtype != np.uint16 or dtest.ndim != 3 or dtest.size == 0:
        raise ValueError("depth_test_u16 must be a non-empty uint16 array [T, H, W]")
    idx = np.ascontiguousarray(test_index, dtype=np.int32).reshape(-1)
    if len(idx) != len(poses):
        raise ValueError("test_index needs one entry per pose")
    return poses, vertices, faces, np.ascontiguousarray(K, dtype=np.float64).reshape(9), dtest, idx


def icp_normal_equations(poses, vertices, faces, K, depth_test_u16, test_index, depth_scale=0.001, max_dist=0.02,
                         min_cos=0.25, pixel_center=0.0, near=0.01, device=None, chunk=None):
    """One accumulation of refine_poses_depth at the given poses: float64 [P, 29] = the upper triangle of A = sum J^T J
    row by row (21), b = sum J^T r (6), the number N of pixels that took part and E = sum r^2.  ``device=None``:
    bp_icp_normal_equations_host; a torch device: bp_icp_normal_equations on it (bit-identical from call to call and
    across ``chunk``).  A test index outside [0, T) gives a row of zeros."""
    from . import _lib
    poses, vertices, faces, Kf, dtest, idx = _icp_args(poses, vertices, faces, K, depth_test_u16, test_index)
    T, H, W = dtest.shape
    P = len(poses)
    out = np.zeros((P, ICP_ACC), np.float64)
    if P == 0:
        return out
    side = _lib.Side(device)
    d_poses, mesh = side.put(poses), (side.put(vertices), len(vertices), side.put(faces), len(faces))
    d_out = side.put(out)
    scan = (_lib.ptr(Kf), side.put(dtest), T, H, W, float(depth_scale), side.put(idx), float(max_dist), float(min_cos),
            float(pixel_center), float(near))
    if device is None:
        side.call("bp_icp_normal_equations", d_poses, P, *mesh, *scan, d_out)
    else:
        side.call("bp_icp_normal_equations", *mesh, d_poses, P, *scan, int(chunk or 0), d_out)
    return side.get(d_out)


def refine_poses_depth(poses, vertices, faces, K, depth_test_u16, test_index, depth_scale=0.001, iterations=8,
                       max_dist=0.02, min_cos=0.25, min_pixels=32, pixel_center=0.0, near=0.01, device=None, chunk=None):
    """Depth refinement of P estimated poses of one mesh -- projective point-to-plane ICP against the test depth image:
    ``(poses_out [P, 3, 4] float64, stats [P, 6] float64)``, stats = (N_first, rms_first, N_last, rms_last,
    iterations_done, status), status an index into ICP_STATUS.  Units are the mesh's (LineMod: metres); test image
    ``test_index[p]`` of ``depth_test_u16`` [T, H, W] uint16 has depth ``raw * depth_scale``, 0 = missing.

    Up to ``iterations`` times:
      1. render the depth z_r of the mesh at the current pose (render_depth, the same conventions);
      2. for every pixel (x, y) whose own render and whose four neighbours (x +- 1, y), (x, y +- 1) are inside the image
         and drawn and whose test depth z_t is not 0: the ray d = ((x + c - cx) / fx, (y + c - cy) / fy, 1), the model
         point q = z_r d (the neighbours' likewise), m = (q(x+1,y) - q(x-1,y)) x (q(x,y+1) - q(x,y-1)); the pixel is
         left out when |m| = 0; n = m / |m| turned so that n.d <= 0; left out when -(n.d) / |d| < ``min_cos`` (grazing
         pixels, internal depth edges) or |z_t - z_r| > ``max_dist`` (0.02 m is a fifth of the smallest LineMod
         diameter); residual r = (z_t - z_r)(n.d), which is (s - q).n with s the observed point on the same ray;
         q_c = q - t (the twist is about the object's origin), J = [q_c x n, n];
      3. A = sum J^T J, b = sum J^T r, N, E = sum r^2, rms = sqrt(E / N);
      4. stop before the step when N < ``min_pixels`` (TOO_FEW), the 6x6 solve finds no pivot (SINGULAR), or the
         solution has |omega| > 0.5 rad or |v| > 4 max_dist (DIVERGED: the pose before that step is kept);
      5. else A xi = b, xi = (omega, v), R <- exp(omega) R, t <- t + v.
    One more accumulation without a step gives N_last and rms_last (for a pose that stopped early they are those of the
    accumulation it stopped at).  A pose whose rms_last exceeds its rms_first is returned as it came, bit for bit, with
    status REJECTED and the first pair repeated as the last; a test index outside [0, T) gives NO_IMAGE and the pose
    unchanged.
    ``device=None``: the host twin bp_refine_depth_host (no GPU needed); a torch device: bp_refine_depth on it, the loop
    over the iterations enqueued without a host round trip, ``chunk`` poses at a time (None: a default that keeps the
    workspaces under 256 MB).  Host and device take the same per-pixel decisions with the same bits and differ only in
    the order of the sums; the device results are bit-identical from call to call and across chunk sizes."""
    from . import _lib
    poses, vertices, faces, Kf, dtest, idx = _icp_args(poses, vertices, faces, K, depth_test_u16, test_index)
    T, H, W = dtest.shape
    P = len(poses)
    out, stats = poses.copy(), np.zeros((P, 6), np.float64)
    if P == 0:
        return out, stats
    side = _lib.Side(device)
    d_poses, mesh = side.put(poses), (side.put(vertices), len(vertices), side.put(faces), len(faces))
    d_out, d_stats = side.put(out), side.put(stats)
    scan = (_lib.ptr(Kf), side.put(dtest), T, H, W, float(depth_scale), side.put(idx), int(iterations), float(max_dist),
            float(min_cos), int(min_pixels), float(pixel_center), float(near))
    if device is None:
        side.call("bp_refine_depth", d_poses, P, *mesh, *scan, d_out, d_stats)
    else:
        side.call("bp_refine_depth", *mesh, d_poses, P, *scan, int(chunk or 0), d_out, d_stats)
    return side.get(d_out).reshape(P, 3, 4), side.get(d_stats)


def refine_keypoints(vertices: np.ndarray, keep: int) -> np.ndarray:
    """``Model3D.refine`` (utils/model.py:29-46): ``len - keep`` times, delete the first point (in row-major pair
    order) of the closest pair.  Two quirks of the reference are kept: the running minimum of a round starts at the
    hard-wired 100.0, and the index to delete is carried over from the previous round (initially 0) -- so when every
    pair is at least 100 apart (millimetre-scale, spread-out points) the previous round's index is deleted again."""
    v = np.array(vertices, dtype=np.float64)
    min_index = 0
    for _ in range(max(0, len(v) - keep)):
        diff = v[:, None, :] - v[None, :, :]
        d = np.sqrt(np.sum(np.square(diff), axis=2))
        d[np.diag_indices(len(v))] = np.inf
        if d.min() < 100.0:
            min_index = int(np.unravel_index(np.argmin(d), d.shape)[0])
        v = np.delete(v, min_index, axis=0)
    return v


def _depth_stack(depth_frames, nrs):
    """(test [T, H, W], index [len(nrs)]) of the depth images of the scored frames ``nrs``; KeyError for a missing one."""
    used = sorted(set(nrs))
    for nr in used:
        if nr not in depth_frames:
            raise KeyError("no depth image for frame %d" % nr)
    test = np.stack([np.asarray(depth_frames[nr]) for nr in used])
    return test, np.array([used.index(nr) for nr in nrs], dtype=np.int32)


def evaluate_results(final_result: List[dict], gt_frames: Dict[int, dict], model_vertices, cam_K, diameter_mm,
                     pixel_thresh: float = 5.0, symmetric: bool = False, device=None, symmetries=None,
                     image_width: int = 640, match_instances: bool = False, faces=None, depth_frames=None,
                     depth_scale: float = 0.001, refine_depth=None):
    """The metric loop of betapose_evaluate.py:204-266.  ``gt_frames[nr]`` = list of ``{'pose': 4x4, 'bbox': [x, y, w, h]}`` (one per ground-truth
    annotation compared; a bare dict is accepted for one).
    Returns dict(mean_add, mean_2d_acc, mean_iou, mean_add_err_mm, n).  ``symmetric``: also ADD-S (add_s_err) --
    ``mean_adds``, the fraction under diameter / 10 (the ADD rule of betapose_evaluate.py:246-249), and
    ``mean_adds_err_mm``.  ``device``: every scored pair's errors in one bp_pose_errors call on that torch device
    instead of numpy.  ``symmetries`` (symmetry_transforms): also BOP's MSSD and MSPD over that set on the same scored
    pairs (pose_errors_sym, on ``device`` when one is given) -- ``ar_mssd``, the mean over theta = 0.05 .. 0.50 of the
    fraction with MSSD < theta * diameter, ``ar_mspd``, the mean over theta = 5 .. 50 of the fraction with
    MSPD < theta * image_width / 640, ``mean_mssd_err_mm`` and ``mean_mspd_err_px``.
    ``match_instances``: a frame whose dict has ``"instances"`` (pipeline.finish_candidate_records, all_instances) is
    scored instance by instance instead of ``result[0]`` against every annotation: each ground-truth entry, in list
    order, takes the still unmatched solved instance whose ``bbox`` has the highest IoU with its box (ties: the lower j);
    the pair is scored at IoU >= 0.5, and an entry without such an instance counts in ``n`` and ``mean_iou`` as a miss
    (with the best IoU left, 0 when no instance is).  A frame without any result is skipped, as it is without the flag.
    ``faces`` [F, 3] (load_ply_mesh, indices into ``model_vertices``) and ``depth_frames`` (frame number -> uint16 [H, W]
    test depth image, ``depth_scale`` metres per count), both given: also BOP's VSD on the same scored pairs
    (pose_errors_vsd, on ``device`` when one is given, with ``cam_K``, BOP_VSD_DELTA and BOP_VSD_TAUS) -- ``ar_vsd``, the
    mean over (tau, theta) in BOP_VSD_TAUS x BOP_VSD_THETAS of the fraction of pairs with err(tau) < theta,
    ``mean_vsd_err``, the mean over pairs and taus, and ``mean_visib_fract``, the mean visible fraction of the scored
    ground-truth annotations (those that render at least one pixel).  A scored frame without a depth image raises
    KeyError.
    ``refine_depth``: a dict of keyword arguments of refine_poses_depth (``{}`` for its defaults; ``faces`` and
    ``depth_frames`` are needed): every scored estimate is refined against its frame's depth image, with ``cam_K`` and on
    ``device`` when one is given, BEFORE any error is computed, so every number above is that of the refined poses.  The
    unrefined pose of each scored frame dict is kept under ``"pose_rgb"`` (4x4; with ``match_instances`` in the scored
    instance's dict) and the refined one written over ``cam_R`` / ``cam_t``.  Added keys: ``refined``, the number of
    scored estimates that took at least one step and kept it, ``rejected``, those returned as they came because the
    residual grew, ``unchanged``, the rest (no step was taken: too few pixels, no image, ``iterations`` 0);
    ``refined + rejected + unchanged`` is the number of scored pairs; ``mean_rms_first`` and ``mean_rms_last``, the mean
    rms residual in metres over the estimates with at least one pixel before and after."""
    ious, gts, ests, nrs, owners = [], [], [], [], []
    for f in final_result:
        nr = int(os.path.basename(f["imgname"])[0:-4])
        if nr not in gt_frames:
            continue
        entries = gt_frames[nr]
        if isinstance(entries, dict):
            entries = [entries]
        if match_instances and "instances" in f:
            if len(f["result"]) < 1:
                continue
            free = [j for j, s in enumerate(f["instances"]) if int(s["status"]) == 0 and len(s["cam_R"]) > 0]
            for gt in entries:
                x, y, w, h = gt["bbox"]
                gt_box = [x, y, x + w, y + h]
                best, bi = -1, 0.0
                for j in free:                                   # ascending j: the first maximum is the lower j
                    i = iou(gt_box, np.asarray(f["instances"][j]["bbox"]).tolist())
                    if best < 0 or i > bi:
                        best, bi = j, i
                ious.append(bi)
                if best >= 0 and bi >= 0.5:
                    free.remove(best)
                    s = f["instances"][best]
                    pose = np.eye(4)
                    pose[:3, :3] = s["cam_R"]
                    pose[:3, 3] = np.asarray(s["cam_t"])[:, 0]
                    gts.append(gt["pose"])
                    ests.append(pose)
                    nrs.append(nr)
                    owners.append(s)
            continue
        for gt in entries:
            if len(f["result"]) < 1 or len(f["result"][0]) < 1:
                continue
            x, y, w, h = gt["bbox"]
            gt_box = [x, y, x + w, y + h]
            pred_box = np.asarray(f["result"][0]["bbox"]).tolist()
            i = iou(gt_box, pred_box)
            ious.append(i)
            pose = np.eye(4)
            pose[:3, :3] = f["cam_R"]
            pose[:3, 3] = np.asarray(f["cam_t"])[:, 0]
            if i >= 0.5:
                gts.append(gt["pose"])
                ests.append(pose)
                nrs.append(nr)
                owners.append(f)
    refine_counts = None
    if refine_depth is not None:
        if faces is None or depth_frames is None:
            raise ValueError("refine_depth needs faces and depth_frames")
        nan = float("nan")
        refine_counts = {"refined": 0, "rejected": 0, "unchanged": 0, "mean_rms_first": nan, "mean_rms_last": nan}
        if len(gts):
            test, index = _depth_stack(depth_frames, nrs)
            new, stats = refine_poses_depth(np.reshape(ests, (-1, 4, 4)), model_vertices, faces, cam_K, test, index, depth_scale,
                                            device=device, **refine_depth)
            for j, owner in enumerate(owners):
                owner["pose_rgb"] = ests[j]
                ests[j] = np.vstack([new[j], [0.0, 0.0, 0.0, 1.0]])
                owner["cam_R"], owner["cam_t"] = ests[j][:3, :3].copy(), ests[j][:3, 3].reshape(3, 1).copy()
            rejected = stats[:, 5] == ICP_STATUS.index("REJECTED")
            moved = ~rejected & (stats[:, 4] > 0)
            seen = stats[:, 0] > 0
            refine_counts.update(refined=int(moved.sum()), rejected=int(rejected.sum()),
                                 unchanged=int((~rejected & ~moved).sum()))
            if seen.any():
                refine_counts.update(mean_rms_first=float(stats[seen, 1].mean()), mean_rms_last=float(stats[seen, 3].mean()))
    if device is None:
        add_errs = [add_err(g, e, model_vertices) * 1000 for g, e in zip(gts, ests)]
        proj = [projection_error_2d(g, e, model_vertices, cam_K) for g, e in zip(gts, ests)]
        adds_errs = [add_s_err(g, e, model_vertices) * 1000 for g, e in zip(gts, ests)] if symmetric else []
    else:
        a, s, pr = pose_errors(np.reshape(gts, (-1, 4, 4)), np.reshape(ests, (-1, 4, 4)), model_vertices, cam_K, device,
                               WANT_ADD | WANT_2D | (WANT_ADDS if symmetric else 0))
        add_errs, proj, adds_errs = list(a * 1000), list(pr), list(s * 1000) if symmetric else []
    adds = [a < diameter_mm / 10 for a in add_errs]
    m = {"mean_add": float(np.mean(adds)) if adds else float("nan"),
         "mean_2d_acc": float(np.mean(np.array(proj) < pixel_thresh)) if proj else float("nan"),
         "mean_iou": float(np.mean(np.array(ious) > 0.5)) if ious else float("nan"),
         "mean_add_err_mm": float(np.mean(add_errs)) if add_errs else float("nan"), "n": len(ious)}
    if refine_counts is not None:
        m.update(refine_counts)
    if symmetric:
        m["mean_adds"] = float(np.mean([a < diameter_mm / 10 for a in adds_errs])) if adds_errs else float("nan")
        m["mean_adds_err_mm"] = float(np.mean(adds_errs)) if adds_errs else float("nan")
    if symmetries is not None:
        mssd, mspd = pose_errors_sym(np.reshape(gts, (-1, 4, 4)), np.reshape(ests, (-1, 4, 4)), model_vertices, cam_K,
                                     symmetries, device)
        mssd_mm, r = mssd * 1000, image_width / 640.0
        nan = float("nan")
        m["ar_mssd"] = float(np.mean([np.mean(mssd_mm < th * diameter_mm) for th in BOP_MSSD_THETAS])) if len(gts) else nan
        m["ar_mspd"] = float(np.mean([np.mean(mspd < th * r) for th in BOP_MSPD_THETAS])) if len(gts) else nan
        m["mean_mssd_err_mm"] = float(np.mean(mssd_mm)) if len(gts) else nan
        m["mean_mspd_err_px"] = float(np.mean(mspd)) if len(gts) else nan
    if faces is not None and depth_frames is not None:
        nan = float("nan")
        m["ar_vsd"] = m["mean_vsd_err"] = m["mean_visib_fract"] = nan
        if len(gts):
            test, index = _depth_stack(depth_frames, nrs)
            err, counts = pose_errors_vsd(np.reshape(gts, (-1, 4, 4)), np.reshape(ests, (-1, 4, 4)), model_vertices, faces,
                                          cam_K, test, index, diameter_mm / 1000.0, depth_scale, device=device)
            m["ar_vsd"] = float(np.mean([[np.mean(err[:, k] < th) for th in BOP_VSD_THETAS] for k in range(err.shape[1])]))
            m["mean_vsd_err"] = float(np.mean(err))
            seen = counts[:, 0] > 0
            if seen.any():
                m["mean_visib_fract"] = float(np.mean(counts[seen, 1] / counts[seen, 0]))
    return m


class Model3D:
    """The two methods of the reference's ``Model3D`` the harness uses (utils/model.py:29-46,79-85;
    betapose_evaluate.py:65-81): ``load(path, scale=...)`` of an ASCII .ply into ``vertices`` and ``refine(total_kp)``."""

    def __init__(self, file_to_load=None):
        self.vertices = None
        if file_to_load:
            self.load(file_to_load)

    def load(self, path, demean=False, scale=1.0):
        self.vertices = load_ply_vertices(path) * scale

    def load_mesh(self, path, scale=1.0):
        """What the renderer (betapose_amd/renderer.py) draws, which ``load`` does not read: ``indices`` [F, 3], ``colors``
        [n, 3] floats in [0, 1] (RGB as the file has them, 0.5 without) and ``bb``, the 8 box corners of
        ``_compute_bbox`` (utils/model.py:50-64), next to ``vertices``."""
        v, f, c = load_ply_colored_mesh(path)
        self.vertices = v * scale
        self.indices = f
        self.colors = c.astype(np.float64) / 255.0
        self.bb = box_corners(self.vertices)
        self.bb_colors = np.array(BOX_CORNER_COLORS)

    def refine(self, total_kp=30, save=False, save_path="test.ply"):
        self.vertices = refine_keypoints(self.vertices, total_kp)
