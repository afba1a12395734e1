"""Cases, operands and plain fp64 references of the SE-block launch forms (tests/test_gpu_se_block.py holds the kernels to
them, tests/test_se_block_host.py checks on the CPU that the cases can tell a wrong kernel from a right one):

  * the scaled skip connection   out = act(conv + bias + R * y[b, c])   (ConvParams::res_scale, three implementations)
  * the pooled epilogue          slab sums of conv + bias over 64 rows  (ConvParams::pool_out)
  * avgpool_partial_kernel       slice sums with per = ceil(HW / P)
  * fc_kernel                    act(bias + W (in_scale * sum of slices))
  * maxpool3s2p1_kernel, pixel_shuffle2_kernel

Everything here is torch / numpy on the CPU; nothing is modified by its users (the builders are cached)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------------------------------------------- scaled skip connection
# N, H, W, Cin, Cout, stride, k.  The convolutions are 1x1 as the four "downsample" layers are, but for the last row.
RS_SHAPES = [
    (3, 10, 8, 64, 128, 1, 1),       # HW = 80: image boundaries fall inside the 64-, 128- and 256-row tiles
    (4, 20, 16, 128, 192, 2, 1),     # 10x8 after stride 2; Cout overhangs the 128-wide tiles
    (2, 7, 5, 96, 64, 1, 1),         # HW = 35, M = 70: two images in one 64-row tile, rows past M
    (7, 3, 3, 32, 64, 1, 1),         # HW = 9: seven images in one tile
    (3, 7, 5, 64, 50, 1, 1),         # Cout % 4 != 0: the element-wise epilogue on every tile (HW = 35: three images in two tiles)
    (3, 10, 8, 256, 128, 1, 1),      # the first row with eight K chunks: the only 1x1 row the file's rule lets run in three K slices
    (3, 9, 11, 96, 128, 1, 3),       # 3x3 (HW = 99): reaches the halo tiles, whose epilogue has no staged scale path (element-wise fallback)
]
# kernel ids of the default build that take a residual with a scale (conv_p3 refuses it; conv_s1 has its own shapes below)
RS_TILES_F32 = ["64x64", "128x64"]
RS_TILES_B3 = ["bd_b3", "bdk2_b3", "pl64_b3", "pl128_b3", "pl128x64_b3", "pl256x128_b3"]
RS_TILES_B3_3X3 = ["halo64_b3", "halo128_b3", "halo64k2_b3"]       # 3x3 / stride 1 only; halo128 needs CoutPad % 128 == 0
RS_TILES_F16 = ["pl64_f16", "pl128_f16", "pl128x64_f16", "pl256x128_f16"]
RS_TILES_F16_3X3 = ["plh128_f16"]
RS_ORDERS = (("relu", False), ("leaky", True))      # the ResNet add before the activation, the shortcut add behind it

# the streaming 1x1 kernel (s1_f16: M >= 2048, HW >= 32)
RS_S1_SHAPES = [
    (26, 10, 8, 256, 256, 1, 1),      # HW = 80: boundaries inside 32-row tiles
    (64, 8, 4, 128, 128, 1, 1),       # HW = 32: tiles align with images, the "next image" clamps at N - 1
    (60, 7, 5, 256, 128, 1, 1),       # HW = 35: every other tile spans two images; M tail of 20 rows
    (26, 20, 16, 1024, 2048, 2, 1),   # the layer4 class: two K halves, 32 column groups
]


def family(tile):
    return "f16" if tile.endswith("_f16") else ("b3" if tile.endswith("_b3") else "f32")


def rs_tiles(shape):
    """Every tile id of the default build that accepts the shape with a scaled residual."""
    N, H, W, Cin, Cout, st, k = shape
    tiles = RS_TILES_F32 + RS_TILES_B3 + RS_TILES_F16
    if k == 3 and st == 1:
        tiles = tiles + [t for t in RS_TILES_B3_3X3 if t != "halo128_b3" or ((Cout + 63) // 64 * 64) % 128 == 0] + RS_TILES_F16_3X3
    return tiles


def k_slices_allowed(shape, tile, splits):
    """tests/test_gpu_conv.py's rule: a launch in `splits` K slices needs 2 * splits chunks of 32; the halo tiles cut K by whole
    32-channel groups, so with fewer groups than slices the launch is the one-slice launch again (a duplicate, dropped)."""
    Cin, k = shape[3], shape[6]
    if splits == 1:
        return True
    if Cin * k * k // 32 < 2 * splits:
        return False
    if ("halo" in tile or tile.startswith("plh")) and Cin // 32 < splits:
        return False
    return True


def rs_params():
    return [(shape, tile, splits) for shape in RS_SHAPES for tile in rs_tiles(shape) for splits in (1, 3)
            if k_slices_allowed(shape, tile, splits)]


def out_hw(H, W, k, st, pad):
    return (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1


def conv_bias64(x_nhwc, w, b, st, pad):
    """fp64 conv + bias, NHWC."""
    y = F.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=st, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def rs_problem(shape, rounded, seed):
    """Operands of a scaled-skip case and the fp64 conv + bias of them.  rounded: x and w are fp16 numbers (the f16 tiles' operands)."""
    N, H, W, Cin, Cout, st, k = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    if rounded:
        x, w = x.half().float(), w.half().float()
    b = torch.randn(Cout, generator=g)
    OH, OW = out_hw(H, W, k, st, k // 2)
    R = torch.randn(N, OH, OW, Cout, generator=g)
    gates = 0.05 + 0.9 * torch.rand(N, Cout, generator=g)          # independent uniform(0.05, 0.95) per image and channel
    y64 = conv_bias64(x, w, b, st, k // 2)
    return x, w, b, R, gates, y64


def rs_seed(shape):
    return 4100 + (RS_SHAPES + RS_S1_SHAPES).index(shape)


def pow2_gates(N, Cout):
    """y[b, c] = 2^-((3 b + c) mod 7): distinct across images and across a thread's four channels; R * y is exact in fp32."""
    b = torch.arange(N).view(N, 1)
    c = torch.arange(Cout).view(1, Cout)
    return torch.pow(2.0, -((3 * b + c) % 7).float())


def scaled_skip_ref(y64, R, gates, act, after):
    """(before, behind) the activation, fp64 NHWC: z = conv + bias (+ R y when the add comes first), out = act(z) (+ R y when it comes last)."""
    r = R.double() * gates.double()[:, None, None, :]
    z = y64 if after else y64 + r
    o = F.leaky_relu(z, 0.1) if act == "leaky" else (F.relu(z) if act == "relu" else z)
    if after:
        o = o + r
    return z, o


def elem_bar(ref, fam):
    """The file's bars (tests/test_gpu_conv.py): |d| <= tol (1 + |ref|), tol = 2e-5 for the fp32 and bf16x3 tiles (_check's default),
    2e-5 max(1, mean |ref|) for the f16 tiles on fp16-rounded operands."""
    tol = 2e-5 * (max(1.0, float(ref.abs().mean())) if fam == "f16" else 1.0)
    return tol * (1 + ref.abs())


def boundary_rows(N, hw):
    """Rows (of the [M, C] output) adjacent to an image boundary: the last row of image b and the first of image b + 1."""
    rows = []
    for b in range(N - 1):
        rows += [(b + 1) * hw - 1, (b + 1) * hw]
    return rows


# ---------------------------------------------------------------------------------------------------------------- pooled epilogue
# N, H, W, Cin, Cout; each as 1x1 and 3x3 (pad 1), stride 1
POOL_SHAPES = [
    (1, 10, 8, 64, 128),      # slabs of 64 and 16 rows
    (1, 7, 5, 96, 100),       # one partial slab; the last N tile has 36 live columns
    (1, 16, 8, 32, 64),       # exact slabs
    (3, 16, 8, 64, 64),       # batch with HW a multiple of 64: slab 2 b + j belongs to image b
]
POOL_TILES = ["64x64", "bd_b3", "bdk2_b3", "pl64_b3", "pl64_f16"]       # the 64x64 tiles of each precision ...
POOL_TILES_3X3 = ["halo64_b3", "halo64k2_b3"]                           # ... and the 3x3-only ones


def pool_params():
    out = []
    for shape in POOL_SHAPES:
        for k in (1, 3):
            for tile in POOL_TILES + (POOL_TILES_3X3 if k == 3 else []):
                for splits in (1, 3):
                    if k_slices_allowed(shape[:5] + (1, k), tile, splits):
                        out.append((shape, k, tile, splits))
    return out


@functools.lru_cache(maxsize=None)
def pool_problem(shape, k, rounded, seed):
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    if rounded:
        x, w = x.half().float(), w.half().float()
    b = torch.randn(Cout, generator=g)
    y64 = conv_bias64(x, w, b, 1, k // 2)
    return x, w, b, y64


def pool_seed(shape, k):
    return 4300 + 2 * POOL_SHAPES.index(shape) + (k == 3)


def slab_sums(rows, slab=64, drop_last=False):
    """Column sums of [M, C] over slabs of `slab` rows -> [ceil(M / slab), C] (fp64).  drop_last: without every slab's last valid row."""
    rows = rows.double()
    M, C = rows.shape
    n = (M + slab - 1) // slab
    out = torch.zeros(n, C, dtype=torch.float64)
    for s in range(n):
        lo, hi = s * slab, min(M, (s + 1) * slab)
        out[s] = rows[lo:hi - (1 if drop_last else 0)].sum(0)
    return out


def slab_rows(M, slab=64):
    return [min(slab, M - s * slab) for s in range((M + slab - 1) // slab)]


# ---------------------------------------------------------------------------------------------------------------- avgpool_partial_kernel
AVGPOOL_HW = [80, 127, 128, 129, 320, 511, 1280, 2048, 2050, 5120]
AVGPOOL_C = [64, 100, 256]
AVGPOOL_N = [1, 3]
AVGPOOL_VIEW = (2, 129, 100, 24, 160)      # N, HW, C, first column, row stride: a view into a wider tensor


def avgpool_parts(HW):
    """The engine's slice count (aux_kernels.hip avgpool_parts), restated."""
    return 64 if HW >= 2048 else (32 if HW >= 512 else (8 if HW >= 128 else 2))


def slice_bounds(HW, P):
    per = (HW + P - 1) // P
    return per, [(p * per, min(HW, p * per + per)) for p in range(P)]


def slice_sums(x, P):
    """x [N, HW, C] -> (sums [N, P, C], sums of |x| [N, P, C]) in fp64, slices of per = ceil(HW / P) pixels; an empty slice sums to 0."""
    x = x.double()
    N, HW, C = x.shape
    _, bounds = slice_bounds(HW, P)
    s = torch.zeros(N, P, C, dtype=torch.float64)
    a = torch.zeros(N, P, C, dtype=torch.float64)
    for p, (lo, hi) in enumerate(bounds):
        if lo < hi:
            s[:, p] = x[:, lo:hi].sum(1)
            a[:, p] = x[:, lo:hi].abs().sum(1)
    return s, a


# ---------------------------------------------------------------------------------------------------------------- fc_kernel
FC_CIN = [64, 256, 260, 512, 516, 2048]
FC_COUT = [1, 64, 67]
FC_PARTS = [1, 2, 7, 64, 80]
FC_ACTS = ["linear", "relu", "sigmoid"]
FC_N = [1, 3]


def fc_staging_groups(Cin, in_parts):
    """fc_kernel's G: the 256 threads split the slice sums G ways while staging the input vector (aux_kernels.hip), restated."""
    c4 = Cin // 4
    return (4 if c4 <= 64 else 2) if (in_parts > 1 and c4 <= 128) else 1


def fc_ref(x, w, b, act, in_scale):
    """x [N, Cin], or [N, parts, Cin] slice sums (then v = in_scale * their sum; in_scale is not applied to a plain vector) -> fp64 [N, Cout]."""
    v = x.double()
    if v.dim() == 3:
        v = v.sum(1) * float(in_scale) if v.shape[1] > 1 else v[:, 0]
    o = v @ w.double().t() + b.double()
    if act == "relu":
        o = F.relu(o)
    elif act == "sigmoid":
        o = torch.sigmoid(o)
    return o


def fc_bar(ref):
    """The project's layer bar (tests/test_gpu_nets.py test_kpd_layers_vs_oracle)."""
    return 3e-5 * float(ref.abs().max()) + 1e-5


@functools.lru_cache(maxsize=None)
def fc_problem(Cin, seed):
    """One input of the largest shape per Cin (the cases slice it) and the largest weights."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(max(FC_N), max(FC_PARTS), Cin, generator=g)
    w = torch.randn(max(FC_COUT), Cin, generator=g) / np.sqrt(Cin)
    b = torch.randn(max(FC_COUT), generator=g)
    return x, w, b


# the engine's `parts` switch: conv -> pool in the epilogue -> fc, against conv -> avgpool -> fc.  N, H, W, Cin, Cout, fc outputs
CHAIN_SHAPES = [(1, 10, 8, 64, 128, 16), (1, 16, 8, 64, 128, 16)]      # HW = 80 (slabs of 64 + 16 against 2 slices of 40), HW = 128 (2 slabs against 8 slices)
CHAIN_TILES = ["64x64", "bd_b3", "pl64_f16"]

# ---------------------------------------------------------------------------------------------------------------- max-pool, pixel shuffle
MAXPOOL_CASES = [(2, 7, 5, 4), (1, 8, 6, 68), (2, 9, 16, 64)]      # N, H, W, C
PIXSHUF_CASES = [(2, 3, 5, 8), (1, 4, 4, 16), (1, 5, 4, 2048)]


@functools.lru_cache(maxsize=None)
def maxpool_input(case, seed=5100):
    """randn - 3: almost every element is negative, so a kernel that padded with 0 instead of -inf is wrong at every border."""
    g = torch.Generator().manual_seed(seed + MAXPOOL_CASES.index(case))
    return torch.randn(*case, generator=g) - 3.0


def maxpool_ref(x_nhwc):
    return F.max_pool2d(x_nhwc.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def maxpool_zero_padded(x_nhwc):
    """What a kernel that padded with zeros would return."""
    xp = F.pad(x_nhwc.permute(0, 3, 1, 2), (1, 1, 1, 1), value=0.0)
    return F.max_pool2d(xp, 3, 2, 0).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def pixshuf_input(case, seed=5200):
    g = torch.Generator().manual_seed(seed + PIXSHUF_CASES.index(case))
    return torch.randn(*case, generator=g)


def pixshuf_ref(x_nhwc):
    return F.pixel_shuffle(x_nhwc.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
