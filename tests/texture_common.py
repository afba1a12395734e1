"""What test_texture_host.py and test_gpu_texture.py share: the textures, the meshes, a numpy restatement of DESIGN.md
3.17 written from its text in the same operation order (numpy does not fuse multiply-adds), and ``CASES``: name ->
function(device, size) -> tuple of arrays, the calls the GPU test repeats on the device and compares byte for byte with
the host's.  Image sizes: 75 x 113 (H W odd: the misaligned fallbacks) and 96 x 128.  Textures are small and awkward."""
import functools

import numpy as np

import raster_common as rc

SIZES = [(75, 113), (96, 128)]
TEXTURE_SIZES = [(1, 1), (7, 1), (5, 3), (8, 8), (64, 32)]        # (Wt, Ht)
LIGHT = (0.3, -0.2, 0.0)
FLAT = (200, 100, 50)       # even channels: c/2 + 1/2 is never an integer, see flat_case


def random_texture(Wt, Ht, seed=5, lo=0, hi=256):
    return np.random.default_rng([seed, Wt, Ht]).integers(lo, hi, size=(Ht, Wt, 3), dtype=np.uint8)


def gradient_texture(Wt=64, Ht=32):
    """Red grows with the column, green with the row, blue is a seeded noise: nothing repeats."""
    t = np.zeros((Ht, Wt, 3), np.uint8)
    t[:, :, 0] = (np.arange(Wt) * 255 // max(Wt - 1, 1))[None, :]
    t[:, :, 1] = (np.arange(Ht) * 255 // max(Ht - 1, 1))[:, None]
    t[:, :, 2] = random_texture(Wt, Ht, 9)[:, :, 2]
    return t


def checkerboard(Wt=64, Ht=32):
    ys, xs = np.mgrid[0:Ht, 0:Wt]
    return np.repeat((((xs + ys) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


# ------------------------------------------------------------------------------------------- restatement of DESIGN.md 3.17
def mips_np(texture):
    """The pyramid as a list of [h, w, 3] uint8 arrays: (a + b + c + d + 2) >> 2 of the 2 x 2 block, the partner index
    clamped to the edge where a dimension is odd, down to 1 x 1."""
    levels = [np.asarray(texture, np.uint8)]
    while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
        s = levels[-1].astype(np.int64)
        h, w = s.shape[:2]
        y0, x0 = 2 * np.arange((h + 1) // 2), 2 * np.arange((w + 1) // 2)
        y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
        a, b = s[y0][:, x0], s[y0][:, x1]
        c, d = s[y1][:, x0], s[y1][:, x1]
        levels.append(((((a + b) + (c + d)) + 2) >> 2).astype(np.uint8))
    return levels


def _sub_area(P, Q, X, n):
    px, py, pz = P[0] - X[0], P[1] - X[1], P[2] - X[2]
    qx, qy, qz = Q[0] - X[0], Q[1] - X[1], Q[2] - X[2]
    cx = py * qz - pz * qy
    cy = pz * qx - px * qz
    cz = px * qy - py * qx
    return (cx * n[0] + cy * n[1]) + cz * n[2]


def _clamp01(w):
    return np.where(w < 0.0, 0.0, np.where(w > 1.0, 1.0, w))


def _wrap01(u):
    u = np.where(u == u, u, 0.0)
    u = np.where(u > 2.0 ** 30, 2.0 ** 30, u)
    u = np.where(u < -2.0 ** 30, -2.0 ** 30, u)
    return u - np.floor(u)


def _plane_uv(n, nd, nn, A, B, C, uv, dx, dy):
    z = nd / ((n[0] * dx + n[1] * dy) + n[2])
    X = (z * dx, z * dy, z)
    a = _sub_area(B, C, X, n) / nn
    b = _sub_area(C, A, X, n) / nn
    c = _sub_area(A, B, X, n) / nn
    return (a * uv[0][0] + b * uv[1][0]) + c * uv[2][0], (a * uv[0][1] + b * uv[1][1]) + c * uv[2][1]


def fragment_np(A, B, C, uv, xs, ys, K, c, ambient, light, Wt, Ht):
    """(u, v, rx, ry, light_w) of the pixels (xs, ys) on the triangle with camera-space vertices A, B, C (float64
    triples) and corner coordinates uv [3][2]: the text of 3.5's fragment and 3.17's footprint, operation by operation."""
    A, B, C = [[float(t) for t in P] for P in (A, B, C)]
    uv = [[float(t) for t in row] for row in np.asarray(uv)]
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    e1 = [B[k] - A[k] for k in range(3)]
    e2 = [C[k] - A[k] for k in range(3)]
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    nd = (n[0] * A[0] + n[1] * A[1]) + n[2] * A[2]
    zmin, zmax = min(A[2], B[2], C[2]), max(A[2], B[2], C[2])
    xs, ys = xs.astype(np.float64), ys.astype(np.float64)
    dx, dy = ((xs + c) - cx) / fx, ((ys + c) - cy) / fy
    with np.errstate(all="ignore"):
        z = nd / ((n[0] * dx + n[1] * dy) + n[2])
        z = np.where(z >= zmin, z, zmin)
        z = np.where(z > zmax, zmax, z)
        X = (z * dx, z * dy, z)
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        assert nn > 0.0
        a = _clamp01(_sub_area(B, C, X, n) / nn)
        b = _clamp01(_sub_area(C, A, X, n) / nn)
        cc = _clamp01(_sub_area(A, B, X, n) / nn)
        total = (a + b) + cc
        ok = total > 0.0
        safe = np.where(ok, total, 1.0)
        wa, wb, wc = (np.where(ok, w / safe, 1.0 / 3.0) for w in (a, b, cc))
        length = float(np.sqrt(nn))
        N = [n[0] / length, n[1] / length, n[2] / length]
        flip = (N[0] * X[0] + N[1] * X[1]) + N[2] * X[2] > 0.0
        Nx, Ny, Nz = (np.where(flip, -N[k], N[k]) for k in range(3))
        lx, ly, lz = light[0] - X[0], light[1] - X[1], light[2] - X[2]
        ll = np.sqrt((lx * lx + ly * ly) + lz * lz)
        lsafe = np.where(ll > 0.0, ll, 1.0)
        diffuse = np.where(ll > 0.0, ((lx / lsafe) * Nx + (ly / lsafe) * Ny) + (lz / lsafe) * Nz, 0.0)
        diffuse = np.where(diffuse > 0.0, diffuse, 0.0)
        light_w = ambient + 0.5 * diffuse
        light_w = np.where(light_w > 1.0, 1.0, light_w)
        u = (wa * uv[0][0] + wb * uv[1][0]) + wc * uv[2][0]
        v = (wa * uv[0][1] + wb * uv[1][1]) + wc * uv[2][1]
        # the footprint: unclamped barycentrics on the plane at the rays of (x, y), (x + 1, y), (x, y + 1)
        dx1, dy1 = (((xs + 1.0) + c) - cx) / fx, (((ys + 1.0) + c) - cy) / fy
        u0, v0 = _plane_uv(n, nd, nn, A, B, C, uv, dx, dy)
        ux, vx = _plane_uv(n, nd, nn, A, B, C, uv, dx1, dy)
        uy, vy = _plane_uv(n, nd, nn, A, B, C, uv, dx, dy1)
        ax, bx = (ux - u0) * float(Wt), (vx - v0) * float(Ht)
        ay, by = (uy - u0) * float(Wt), (vy - v0) * float(Ht)
        rx, ry = ax * ax + bx * bx, ay * ay + by * by
    return u, v, rx, ry, light_w


def level_np(rx, ry, levels):
    """The number of l < levels - 1 with rx > 4^l or ry > 4^l (a comparison with a NaN is false)."""
    level = np.zeros(np.shape(rx), np.int64)
    with np.errstate(invalid="ignore"):
        for l in range(levels - 1):
            level += ((rx > 4.0 ** l) | (ry > 4.0 ** l)).astype(np.int64)
    return level


def sample_np(tex, u, v):
    """Bilinear sample of one level [h, w, 3] in 8-bit fixed point, wrap mode repeat: int64 [..., 3]."""
    h, w = tex.shape[:2]
    s = _wrap01(u) * float(w) - 0.5
    t = (1.0 - _wrap01(v)) * float(h) - 0.5
    si, ti = np.floor(256.0 * s).astype(np.int64), np.floor(256.0 * t).astype(np.int64)
    x0, fx = (si >> 8), (si & 255)[..., None]          # numpy's >> and & on negative integers are floor and modulo
    y0, fy = (ti >> 8), (ti & 255)[..., None]
    T = tex.astype(np.int64)
    c00, c10 = T[y0 % h, x0 % w], T[y0 % h, (x0 + 1) % w]
    c01, c11 = T[(y0 + 1) % h, x0 % w], T[(y0 + 1) % h, (x0 + 1) % w]
    return ((c00 * (256 - fx) + c10 * fx) * (256 - fy) + (c01 * (256 - fx) + c11 * fx) * fy + 32768) >> 16


def winners(pose, v, f, K, size, c, near=0.01):
    """(face [H, W] int, -1 where nothing is drawn; depth [H, W] float32): every face rendered alone by the depth
    rasteriser (coverage and depth are not what these tests are about), nearest first, then the lowest face."""
    from betapose_amd import metrics
    alone = np.stack([metrics.render_depth(pose[None], v, f[k:k + 1], K, size, None, c, near)[0][0] for k in range(len(f))])
    key = np.where(alone > 0, alone, np.float32(np.inf))
    face = key.argmin(axis=0)
    best = key.min(axis=0)
    drawn = np.isfinite(best)
    return np.where(drawn, face, -1), np.where(drawn, best, np.float32(0)).astype(np.float32)


def render_np(pose, v, f, uv, texture, K, size, c=0.0, ambient=0.5, light=(0.0, 0.0, 0.0), mip=True, want_rho=False):
    """The textured image [H, W, 3] uint8 of one pose by the restatement (and, asked for, rho^2 = max(rx, ry) [H, W],
    NaN where nothing is drawn)."""
    pyramid = mips_np(texture)
    Ht, Wt = pyramid[0].shape[:2]
    levels = len(pyramid) if mip else 1
    face, _ = winners(pose, v, f, K, size, c)
    out = np.zeros(tuple(size) + (3,), np.uint8)
    rho2 = np.full(tuple(size), np.nan)
    # ((R00 x + R01 y) + R02 z) + t0, as rs_transform sums them
    X = np.stack([((pose[k, 0] * v[:, 0] + pose[k, 1] * v[:, 1]) + pose[k, 2] * v[:, 2]) + pose[k, 3] for k in range(3)], axis=1)
    for k in range(len(f)):
        ys, xs = np.nonzero(face == k)
        if not len(xs):
            continue
        A, B, C = X[f[k, 0]], X[f[k, 1]], X[f[k, 2]]
        u, vv, rx, ry, light_w = fragment_np(A, B, C, uv[k], xs, ys, K, c, ambient, light, Wt, Ht)
        level = level_np(rx, ry, levels)
        base = np.zeros((len(xs), 3), np.int64)
        for l in range(levels):
            on = level == l
            if on.any():
                base[on] = sample_np(pyramid[l], u[on], vv[on])
        val = np.floor(light_w[:, None] * base.astype(np.float64) + 0.5)
        out[ys, xs] = np.clip(val, 0, 255).astype(np.uint8)
        with np.errstate(invalid="ignore"):
            rho2[ys, xs] = np.where(rx > ry, rx, ry)
    return (out, rho2) if want_rho else out


# ------------------------------------------------------------------------------------------------------------- meshes
QUAD_UV = np.array([[0.0, 1.0], [1.0, 1.0], [1.0, 0.0], [0.0, 0.0]])     # corner 0 is the image's top left
QUAD_FACES = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def window_quad(x0, y0, wpx, hpx, size, z=2.0, c=0.0):
    """The fronto-parallel quad whose texture spans exactly the pixels x0 .. x0 + wpx - 1 by y0 .. y0 + hpx - 1: its
    corners lie half a pixel outside the centres of the window's border pixels.  (vertices, faces, uv [2, 3, 2])."""
    v, f = rc.pixel_quad([(x0 - 0.5, y0 - 0.5), (x0 + wpx - 0.5, y0 - 0.5), (x0 + wpx - 0.5, y0 + hpx - 0.5), (x0 - 0.5, y0 + hpx - 0.5)],
                         [z] * 4, size, c)
    return v, f, np.ascontiguousarray(QUAD_UV[f])


def tilted_quad(size, angle=60.0, z=3.0, half=(1.0, 0.6)):
    """A quad turned ``angle`` degrees about the vertical axis through its middle, at depth z: (vertices, faces, uv,
    pose)."""
    a = np.radians(angle)
    v = np.array([[-half[0], -half[1], 0.0], [half[0], -half[1], 0.0], [half[0], half[1], 0.0], [-half[0], half[1], 0.0]])
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    pose = np.hstack([R, [[0.05], [-0.03], [z]]])
    return v, QUAD_FACES.copy(), np.ascontiguousarray(QUAD_UV[QUAD_FACES]), pose


EYE = np.hstack([np.eye(3), np.zeros((3, 1))])


def corner_uv(F, seed=7):
    """Seeded corner coordinates in [-0.5, 1.5): seams everywhere and the wrap in use."""
    return np.random.default_rng(seed).uniform(-0.5, 1.5, size=(F, 3, 2))


def far_quad(size):
    """The minification view: the 64 x 32 texture over a window of a third of its size, so one pixel step is three
    texels on both axes (rho = 3: level 2, well away from the thresholds at 2 and 4)."""
    H, W = size
    return window_quad(W // 2 - 10, H // 2 - 5, 64.0 / 3.0, 32.0 / 3.0, size)


# ------------------------------------------------------------------------------------------------------------- cases
def _identity_case(Wt, Ht):
    def run(device, size):
        from betapose_amd import metrics
        v, f, uv = window_quad(11, 7, Wt, Ht, size)
        return metrics.render_color(EYE[None], v, f, None, rc.camera(size), size, device, ambient=1.0, uv=uv,
                                    texture=random_texture(Wt, Ht, lo=96, hi=160), mip=False)
    return run


def _flat_case(Wt, Ht, mip):
    def run(device, size):
        from betapose_amd import metrics
        v, f = rc.torus()
        tex = np.tile(np.array(FLAT, np.uint8), (Ht, Wt, 1))
        return metrics.render_color(rc.poses_for("torus", size=size), v, f, None, rc.camera(size), size, device, light=LIGHT,
                                    uv=corner_uv(len(f)), texture=tex, mip=mip)
    return run


def _minify_case(mip):
    def run(device, size):
        from betapose_amd import metrics
        v, f, uv = far_quad(size)
        return metrics.render_color(EYE[None], v, f, None, rc.camera(size), size, device, ambient=1.0, uv=uv,
                                    texture=checkerboard(), mip=mip)
    return run


def _perspective_case(c):
    def run(device, size):
        from betapose_amd import metrics
        v, f, uv, pose = tilted_quad(size)
        return metrics.render_color(pose[None], v, f, None, rc.camera(size), size, device, pixel_center=c, light=LIGHT, uv=uv,
                                    texture=gradient_texture())
    return run


def bad_uv(uv):
    """Face 1's corners set to NaN, +inf, -inf and 1e300; face 0 untouched."""
    uv = uv.copy()
    uv[1] = [[np.nan, 0.25], [np.inf, -np.inf], [1e300, 0.5]]
    return uv


def _wrap_case(kind):
    def run(device, size):
        from betapose_amd import metrics
        v, f, uv, pose = tilted_quad(size, angle=40.0)
        uv = {"plain": uv, "shifted": uv + [1.0, -2.0], "bad": bad_uv(uv)}[kind]
        return metrics.render_color(pose[None], v, f, None, rc.camera(size), size, device, light=LIGHT, uv=uv,
                                    texture=random_texture(5, 3))
    return run


def _into_case(textured_first):
    """The icosphere textured and the box vertex-coloured, three poses each into two images, one after the other."""
    def run(device, size):
        from betapose_amd import metrics
        import render_color_common as cc
        (sv, sf, _, ps), (bv, bf, bc, pb), _ = cc.two_mesh_scene()
        K = rc.camera(size)
        index = np.array([0, 1, 1], np.int32)
        pb = pb.copy()
        pb[:, 3] = ps[:, 3] + [0.7, 0.2, -0.2]       # the box beside the sphere and a little nearer: it hides a part of it
        sp = np.stack([ps, ps, ps])
        sp[2, 0, 3] += 0.3
        bp = np.stack([pb, pb, pb])
        bp[2, 0, 3] -= 0.3                           # ... and once behind it
        bp[2, 2, 3] += 0.6
        tex = dict(uv=corner_uv(len(sf), 3), texture=random_texture(8, 8))
        if textured_first:
            first = metrics.render_color(sp, sv, sf, None, K, size, device, image_index=index, images=2, **tex)
            second = metrics.render_color(bp, bv, bf, bc, K, size, device, image_index=index, images=2, into=first[:2])
        else:
            first = metrics.render_color(bp, bv, bf, bc, K, size, device, image_index=index, images=2)
            second = metrics.render_color(sp, sv, sf, None, K, size, device, image_index=index, images=2, into=first[:2], **tex)
        return first + second
    return run


def _tie_case(textured_last):
    """One triangle drawn twice at exactly the same depth, red by vertex colours and blue by a flat texture."""
    def run(device, size):
        from betapose_amd import metrics
        tri = np.array([[-0.5, -0.4, 2.0], [0.6, -0.3, 2.0], [0.0, 0.5, 2.0]])
        f = np.array([[0, 1, 2]], np.int32)
        K = rc.camera(size)
        red = dict(colors=np.tile(np.array([254, 0, 0], np.uint8), (3, 1)))
        blue = dict(colors=None, uv=np.zeros((1, 3, 2)), texture=np.tile(np.array([0, 0, 254], np.uint8), (1, 1, 1)))
        a, b = (red, blue) if textured_last else (blue, red)
        first = metrics.render_color(EYE[None], tri, f, K=K, size=size, device=device, ambient=1.0, **a)
        return metrics.render_color(EYE[None], tri, f, K=K, size=size, device=device, ambient=1.0, into=first[:2], **b)
    return run


CASES = {}
for _wt, _ht in TEXTURE_SIZES:
    CASES["identity-%dx%d" % (_wt, _ht)] = _identity_case(_wt, _ht)
for _wt, _ht in ((8, 8), (1, 1)):
    for _mip in (True, False):
        CASES["flat-%dx%d-%s" % (_wt, _ht, "mip" if _mip else "base")] = _flat_case(_wt, _ht, _mip)
CASES["minify-mip"] = _minify_case(True)
CASES["minify-base"] = _minify_case(False)
CASES["perspective-0.0"] = _perspective_case(0.0)
CASES["perspective-0.5"] = _perspective_case(0.5)
for _kind in ("plain", "shifted", "bad"):
    CASES["wrap-" + _kind] = _wrap_case(_kind)
CASES["into-textured-first"] = _into_case(True)
CASES["into-textured-last"] = _into_case(False)
CASES["tie-textured-last"] = _tie_case(True)
CASES["tie-textured-first"] = _tie_case(False)


@functools.lru_cache(maxsize=None)
def host(name, size):
    """The host twin's result of a case, computed once per session and read-only."""
    out = CASES[name](None, tuple(size))
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------- synthesiser
SYNTH_SIZE = (75, 113)
SYNTH_SEED = 3


def synth_meshes(textured=True):
    """(target, occluder) in metres: the icosphere, textured (or with the same vertex colours alone), and the torus with
    vertex colours."""
    import synth_common as sc
    sv, sf = rc.icosphere()
    tv, tf = rc.torus()
    target = (sv * 0.05, sf, sc.vertex_colors(len(sv), 11))
    if textured:
        target = target + (corner_uv(len(sf), 13), gradient_texture())
    return target, (tv * 0.03, tf, sc.vertex_colors(len(tv), 12))


def synth_scenes(textured, n=3, device=None, first_scene=0):
    from betapose_amd import synth
    target, occluder = synth_meshes(textured)
    return synth.synthesize_scenes(target, [occluder], rc.camera(SYNTH_SIZE), SYNTH_SIZE, n, SYNTH_SEED,
                                   sensor=dict(noise_k=0, hole_p=0), first_scene=first_scene, device=device)


def synth_multi(textured, n=3, device=None, first_scene=0):
    from betapose_amd import synth
    target, occluder = synth_meshes(textured)
    return synth.synthesize_multi([target, occluder], rc.camera(SYNTH_SIZE), SYNTH_SIZE, n, SYNTH_SEED, min_visib=0.1,
                                  sensor=dict(noise_k=0, hole_p=0), first_scene=first_scene, device=device)


@functools.lru_cache(maxsize=None)
def host_synth(kind, textured):
    out = (synth_scenes if kind == "scenes" else synth_multi)(textured)
    for a in out.values():
        a.setflags(write=False)
    return out
