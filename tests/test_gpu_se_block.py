"""The launch forms of the key-point detector's SE blocks, each alone (cases, references and their premises:
tests/se_block_common.py, tests/test_se_block_host.py):

  * ConvParams::res_scale -- the skip connection times a gate per image and channel -- in its three implementations: the
    element-wise epilogue (conv_dev.h epilogue_store), the staged ResScaleRows path of the kernels that define BP_EP_RES_SCALE
    (conv_igemm.hip, conv_pl.hip) and the streaming 1x1 kernel's two-image gate tile in LDS (conv_s1.hip);
  * ConvParams::pool_out -- the global average pool as 64-row slab sums in the producing convolution's epilogue;
  * avgpool_partial_kernel and fc_kernel, and the engine's switch of `in_parts` between the two pools;
  * maxpool3s2p1_kernel and pixel_shuffle2_kernel with their operand-plane stores.

Which implementation a scaled-skip launch takes follows from the kernels' eligibility code (conv_tail.inc: ep_rs = the kernel
defines BP_EP_RES_SCALE and the store is NHWC; ep_vec_ok needs Cout % 4 == 0):
  64x64, 128x64 (conv_igemm_kernel), bd_b3, bdk2_b3 (conv_igemm_h / bdk2), pl*_b3, pl*_f16, plh128_f16 (conv_pl_kernel)
      -> staged ResScaleRows when Cout % 4 == 0, element-wise when not (the Cout = 50 row)
  halo64_b3, halo128_b3, halo64k2_b3 (conv_halo.hip: no BP_EP_RES_SCALE)   -> element-wise always (the 3x3 row)
  s1_f16 (conv_s1.hip)                                                     -> the gate tile in LDS
Three of the four oracles are bit identities and need no tolerance; the fourth uses the bars tests/test_gpu_conv.py already has."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import se_block_common as sb  # noqa: E402
from betapose_amd import _lib, ops  # noqa: E402
from test_gpu_conv import F16R_SENTINEL, _bits_differ, _check, _f16r_sentinel, _planes_to_f32  # noqa: E402


def _untouched(buf):
    return not bool((buf.view(torch.int32) != F16R_SENTINEL).any())


def _gate_check(out, ref64, fam, what):
    """Oracle 4's bar: _check's default for the fp32 and bf16x3 tiles, 2e-5 max(1, mean |ref|) for the f16 tiles (fp16-rounded operands)."""
    tol = 2e-5 * (max(1.0, float(ref64.abs().mean())) if fam == "f16" else 1.0)
    d = (out.cpu().double() - ref64).abs()
    print("%s: max |d| %.3e, worst d / bar %.3f" % (what, float(d.max()), float((d / (tol * (1 + ref64.abs()))).max())))
    _check(out.cpu(), ref64.float(), tol=tol)


def _rs_check(cuda, monkeypatch, shape, tile, splits):
    N, H, W, Cin, Cout, st, k = shape
    fam = sb.family(tile)
    x, w, b, R, gates, y64 = sb.rs_problem(shape, fam == "f16", sb.rs_seed(shape))
    xd, Rd, gd = x.to(cuda), R.to(cuda), gates.to(cuda)
    ones = torch.ones(N, Cout, device=cuda)
    p2 = sb.pow2_gates(N, Cout)
    Rp2 = R * p2[:, None, None, :]
    assert torch.equal(Rp2.double(), R.double() * p2.double()[:, None, None, :])      # the pre-multiplication is exact
    p2d, Rp2d = p2.to(cuda), Rp2.to(cuda)
    R16d = R.half().float().to(cuda)
    monkeypatch.delenv("BP_CONV_F16R", raising=False)
    for act, after in sb.RS_ORDERS:
        kw = dict(stride=st, pad=k // 2, act=act, res_after_act=after, tile=tile, splits=splits)
        what = "%s %s splits=%d %s add %s the activation" % ("x".join(map(str, shape)), tile, splits, act, "after" if after else "before")
        run = lambda **more: ops.conv2d_nhwc(xd, w, b, **kw, **more)      # noqa: E731
        # 1. gates of exactly 1.0: the launch without a scale, bit for bit
        plain = run(res=Rd)
        one = [run(res=Rd, res_scale=ones) for _ in range(2)]
        assert torch.equal(one[0], plain), what + ": gates of 1.0 change the output, " + _bits_differ(one[0], plain)
        assert torch.equal(one[1], one[0]), what
        # 2. power-of-two gates: the launch without a scale on the pre-multiplied residual, bit for bit (same tile, same K cut: `splits`
        # and the shape are the same, and conv_launch_of does not look at the residual)
        pre = run(res=Rp2d)
        two = [run(res=Rd, res_scale=p2d) for _ in range(2)]
        assert torch.equal(two[0], pre), what + ": scaled residual != pre-multiplied residual, " + _bits_differ(two[0], pre)
        assert torch.equal(two[1], two[0]), what
        assert not torch.equal(two[0], plain), what                               # (the gates were applied at all)
        # 4. random gates against fp64
        _, ref = sb.scaled_skip_ref(y64, R, gates, act, after)
        rnd = [run(res=Rd, res_scale=gd) for _ in range(2)]
        _gate_check(rnd[0], ref, fam, what)
        assert torch.equal(rnd[1], rnd[0]), what
        if fam != "f16":
            continue
        # 3. BP_CONV_F16R=1 with gates (res16 + res_scale): the plain f16 launch given R16 = fp16(R) widened and the same gates, bit for bit;
        # with planes and a sentinel-filled out=, the same plane and no fp32 element stored
        A, plA = run(res=R16d, res_scale=gd, planes=True)
        monkeypatch.setenv("BP_CONV_F16R", "1")
        B = [run(res=Rd, res_scale=gd) for _ in range(2)]
        Cs = []
        for _ in range(2):
            buf = _f16r_sentinel(A.shape, cuda)
            ret, pl = run(res=Rd, res_scale=gd, planes=True, out=buf)
            assert ret is buf
            Cs.append((buf, pl))
        monkeypatch.delenv("BP_CONV_F16R")
        assert torch.equal(B[0], A), what + ": res16 + res_scale launch != fp32-residual launch, " + _bits_differ(B[0], A)
        assert torch.equal(B[1], B[0]), what
        assert float((B[0] - rnd[0]).abs().max()) > 1e-6, what                   # (the plane was really read: R is not made of fp16 numbers)
        assert torch.equal(Cs[0][1], plA), what + ": plane of the f16r launch != plane of the fp32 launch, " + _bits_differ(Cs[0][1], plA)
        assert torch.equal(Cs[1][1], Cs[0][1]), what
        for buf, _ in Cs:
            assert _untouched(buf), what + ": skip_f32 launch stored fp32 elements"
        assert torch.equal(_planes_to_f32(plA, "f16"), A.half().float()), what


@pytest.mark.parametrize("shape,tile,splits", sb.rs_params(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_res_scale(cuda, monkeypatch, shape, tile, splits):
    """The scaled skip connection on every tile of the default build that takes it, one K slice and three, both add orders."""
    _rs_check(cuda, monkeypatch, shape, tile, splits)


@pytest.mark.parametrize("shape", sb.RS_S1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_res_scale_s1(cuda, monkeypatch, shape):
    """... and on the streaming 1x1 kernel: the gates of the tile's first image and the next one ride in LDS behind the skip-connection tile.
    (K = 1 024: the LDS plan with a scale differs from the one without in `rbuf` and the offsets behind it alone -- NL = min(nl, 2), MS, NG
    and the grid do not depend on it -- so the bit identities hold there too, as they do for res16 in tests/test_gpu_conv.py.)"""
    monkeypatch.setenv("BP_S1_K512", "1")
    _rs_check(cuda, monkeypatch, shape, "s1_f16", 1)


def test_res_scale_needs_a_residual(cuda):
    x = torch.randn(1, 4, 4, 32)
    with pytest.raises(_lib.BetaposeHipError, match="residual"):
        ops.conv2d_nhwc(x.to(cuda), torch.randn(64, 32, 1, 1), None, res_scale=torch.ones(1, 64, device=cuda))


# ---------------------------------------------------------------------------------------------------------------- pooled epilogue
@pytest.mark.parametrize("shape,k,tile,splits", sb.pool_params(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pool_in_epilogue(cuda, shape, k, tile, splits):
    N, H, W, Cin, Cout = shape
    fam = sb.family(tile)
    x, w, b, y64 = sb.pool_problem(shape, k, fam == "f16", sb.pool_seed(shape, k))
    M = N * H * W
    slabs = (M + 63) // 64
    kw = dict(pad=k // 2, tile=tile, splits=splits)
    xd = x.to(cuda)
    out = ops.conv2d_nhwc(xd, w, b, **kw)
    bufs = []
    for _ in range(2):
        buf = _f16r_sentinel((slabs + 1, Cout), cuda)          # one slab row too long
        out_p, ret = ops.conv2d_nhwc(xd, w, b, pool=buf, **kw)
        assert ret is buf
        assert torch.equal(out_p, out), "pool=True changes the output, " + _bits_differ(out_p, out)
        written = buf.view(torch.int32) != F16R_SENTINEL
        assert bool(written[:slabs].all()), "%d of %d pool elements not written" % (int((~written[:slabs]).sum()), slabs * Cout)
        assert not bool(written[slabs:].any()), "the launch wrote past ceil(M / 64) slab rows"
        bufs.append(buf)
    assert torch.equal(bufs[1].view(torch.int32), bufs[0].view(torch.int32))      # (bits: the spare row holds the sentinel NaN)
    pool =bufs[0][:slabs].cpu().double()
    nv = torch.tensor(sb.slab_rows(M), dtype=torch.float64)[:, None]
    # against the launch's own fp32 output: the rounding of an fp32 sum of nvalid terms plus the bias product
    rows = out.cpu().reshape(M, Cout)
    own = sb.slab_sums(rows)
    lim = 2.0 ** -23 * nv * (sb.slab_sums(rows.abs()) + nv * b.double().abs()[None, :])
    d = (pool - own).abs()
    print("pool - sum(out): worst d / bound %.3f" % float((d / lim).max()))
    assert bool((d <= lim).all()), "max |pool - sum(out)| %.3e" % float(d.max())
    # against fp64 conv + bias: a sum of nvalid element errors -- the sum of the rows' element bars
    ref_rows = y64.reshape(M, Cout)
    bar = sb.slab_sums(sb.elem_bar(ref_rows, fam))
    d = (pool - sb.slab_sums(ref_rows)).abs()
    print("pool - fp64: worst d / bar %.3f" % float((d / bar).max()))
    assert bool((d <= bar).all()), "max |pool - ref| %.3e" % float(d.max())


@pytest.mark.parametrize("why,shape,kw", [
    ("batch > 1 with HW = 80: a slab spans two images", (3, 10, 8, 64, 128), dict(tile="64x64")),
    ("a 128-row tile (fp32)", (1, 10, 8, 64, 128), dict(tile="128x64")),
    ("a 128-row tile (f16 planes)", (1, 10, 8, 64, 128), dict(tile="pl128_f16")),
    ("a 128-row tile (bf16x3 planes)", (1, 10, 8, 64, 128), dict(tile="pl128x64_b3")),
    ("an activation", (1, 10, 8, 64, 128), dict(tile="64x64", act="relu")),
    ("a residual", (1, 10, 8, 64, 128), dict(tile="pl64_f16", res=True)),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_pool_in_epilogue_is_refused(cuda, why, shape, kw):
    """Where the engine's precondition does not hold the hook fails cleanly and launches nothing: output and pool buffer keep the sentinel."""
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(4500)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / 8
    b = torch.randn(Cout, generator=g)
    kw = dict(kw)
    if kw.pop("res", False):
        kw["res"] = torch.randn(N, H, W, Cout, generator=g).to(cuda)
    out = _f16r_sentinel((N, H, W, Cout), cuda)
    buf = _f16r_sentinel(((N * H * W + 63) // 64 + 1, Cout), cuda)
    with pytest.raises(_lib.BetaposeHipError, match="average pool"):
        ops.conv2d_nhwc(x.to(cuda), w, b, out=out, pool=buf, **kw)
    torch.cuda.synchronize()
    assert _untouched(out) and _untouched(buf), why
    assert torch.isfinite(ops.conv2d_nhwc(x.to(cuda), w, b, out=out, **kw)).all()      # (the same launch without the pool runs)


# ---------------------------------------------------------------------------------------------------------------- avgpool_partial_kernel, fc_kernel
def _avgpool_check(cuda, x, wide=None, c0=0):
    """x [N, HW, C] (CPU); wide: the tensor x is a view of (columns c0 .. c0 + C)."""
    N, HW, C = x.shape
    P = sb.avgpool_parts(HW)
    per, _ = sb.slice_bounds(HW, P)
    src = (wide if wide is not None else x).to(cuda)
    outs = []
    for _ in range(2):
        buf = _f16r_sentinel((N, P, C), cuda)
        ret, parts = ops.avgpool_parts(src, channels=C, col0=c0, out=buf)
        assert ret is buf and parts == P
        outs.append(buf)
    assert bool((outs[0].view(torch.int32) != F16R_SENTINEL).all()), "slices left unwritten"
    assert torch.equal(outs[1], outs[0])
    ref, mag = sb.slice_sums(x, P)
    lim = 2.0 ** -24 * per * mag                 # the fp32 summation bound; an empty slice must be exactly 0
    d = (outs[0].cpu().double() - ref).abs()
    assert bool((d <= lim).all()), "N=%d HW=%d C=%d: max |d| %.3e, worst d / bound %.3f" % (N, HW, C, float(d.max()), float((d / lim.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("HW", sb.AVGPOOL_HW)
def test_avgpool_slice_sums(cuda, HW):
    g = torch.Generator().manual_seed(4600 + HW)
    full = torch.randn(max(sb.AVGPOOL_N), HW, max(sb.AVGPOOL_C), generator=g)
    for C in sb.AVGPOOL_C:
        for N in sb.AVGPOOL_N:
            _avgpool_check(cuda, full[:N, :, :C].contiguous())
    _, parts = ops.avgpool_parts(full[:1].to(cuda))
    assert parts == sb.avgpool_parts(HW)


def test_avgpool_view_into_a_wider_tensor(cuda):
    """in_ld > C: the columns outside the view hold 1e30 -- one of them read, and no bound holds."""
    N, HW, C, c0, ld = sb.AVGPOOL_VIEW
    g = torch.Generator().manual_seed(4700)
    x = torch.randn(N, HW, C, generator=g)
    wide = torch.full((N, HW, ld), 1e30)
    wide[:, :, c0:c0 + C] = x
    _avgpool_check(cuda, x, wide=wide, c0=c0)


@pytest.mark.parametrize("Cin", sb.FC_CIN)
def test_fc(cuda, Cin):
    """Every staging branch of fc_kernel (G = 4 / 2 / 1, four LDS copies of the vector or one), every activation, Cout below and off the
    eight neurons of a block; and row b of an N = 3 launch is the N = 1 launch of that row, bit for bit."""
    x, w, b = sb.fc_problem(Cin, 4800 + Cin)
    xd = x.to(cuda)
    worst = 0.0
    for Cout in sb.FC_COUT:
        for parts in sb.FC_PARTS:
            in_scale = 1.0 / np.sqrt(parts) if parts > 1 else 0.5      # (a plain vector is not scaled: 0.5 must have no effect)
            xin = xd[:, :parts] if parts > 1 else xd[:, 0]
            for act in sb.FC_ACTS:
                what = "Cin=%d Cout=%d in_parts=%d %s" % (Cin, Cout, parts, act)
                ref = sb.fc_ref(x[:, :parts], w[:Cout], b[:Cout], act, in_scale)
                bar = sb.fc_bar(ref)
                out3 = ops.fc(xin, w[:Cout], b[:Cout], act=act, in_scale=in_scale)
                d = float((out3.cpu().double() - ref).abs().max())
                worst = max(worst, d / bar)
                assert d <= bar, what + ": max |d| %.3e > %.3e" % (d, bar)
                for r in range(x.shape[0]):
                    out1 = ops.fc(xin[r:r + 1], w[:Cout], b[:Cout], act=act, in_scale=in_scale)
                    assert torch.equal(out1[0], out3[r]), what + ": row %d of the N = 3 launch != its N = 1 launch, " % r + _bits_differ(out1[0], out3[r])
    print("fc Cin=%d: worst d / bar %.3f" % (Cin, worst))


@pytest.mark.parametrize("tile", sb.CHAIN_TILES)
@pytest.mark.parametrize("shape", sb.CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_fc_chain(cuda, shape, tile):
    """The engine's `in_parts` switch (engine.cpp run_op_unfused OP_FC): ceil(HW / 64) slab sums when the pool rode in the conv's epilogue,
    avgpool_parts(HW) slice sums from the separate kernel -- both are the mean."""
    N, H, W, Cin, Cout, F = shape
    HW = H * W
    fam = sb.family(tile)
    g = torch.Generator().manual_seed(4900 + HW)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / np.sqrt(Cin)
    if fam == "f16":
        x, w = x.half().float(), w.half().float()
    b = torch.randn(Cout, generator=g)
    fw = torch.randn(F, Cout, generator=g) / np.sqrt(Cout)
    fb = torch.randn(F, generator=g)
    mean = sb.conv_bias64(x, w, b, 1, 0).reshape(N, HW, Cout).mean(1)
    ref = sb.fc_ref(mean, fw, fb, "relu", 1.0)
    bar = sb.fc_bar(ref)
    # A: the pool in the epilogue
    out, pool = ops.conv2d_nhwc(x.to(cuda), w, b, tile=tile, pool=True)
    assert pool.shape == ((HW + 63) // 64, Cout)
    a = ops.fc(pool[None], fw, fb, act="relu", in_scale=1.0 / HW)
    # B: the separate kernel on the same convolution's output
    sums, P = ops.avgpool_parts(out)
    assert P == sb.avgpool_parts(HW)
    assert P != pool.shape[0] or not torch.equal(sums[0], pool)      # (another partition of the pixels: HW = 80 is 64 + 16 against 40 + 40)
    bb = ops.fc(sums, fw, fb, act="relu", in_scale=1.0 / HW)
    da, db = float((a.cpu().double() - ref).abs().max()), float((bb.cpu().double() - ref).abs().max())
    print("chain %s HW=%d: A %.3e B %.3e bar %.3e" % (tile, HW, da, db, bar))
    assert da <= bar and db <= bar, (da, db, bar)
    assert float(ref.abs().max()) > 0.1           # (the ReLU left something to compare)


# ---------------------------------------------------------------------------------------------------------------- max-pool, pixel shuffle
def _aux_with_planes(fn, xd, ref):
    out = fn(xd)                                   # no planes: nothing goes through the null plane pointer
    assert torch.equal(out.cpu(), ref), _bits_differ(out.cpu(), ref)
    o1, p1 = fn(xd, planes="f16")
    assert torch.equal(o1, out) and torch.equal(_planes_to_f32(p1, "f16"), out.half().float())      # the plane = RNE fp16 of the output
    o3, p3 = fn(xd, planes="b3")
    assert torch.equal(o3, out) and torch.equal(_planes_to_f32(p3, "b3"), out)                      # the three planes ARE the output, exactly
    assert float((out.half().float() != out).float().mean()) > 0.5                                  # (so the two plane checks differ)


@pytest.mark.parametrize("case", sb.MAXPOOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_maxpool3s2p1(cuda, case):
    x = sb.maxpool_input(case)
    _aux_with_planes(ops.maxpool3s2p1, x.to(cuda), sb.maxpool_ref(x))


@pytest.mark.parametrize("case", sb.PIXSHUF_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pixel_shuffle2(cuda, case):
    x = sb.pixshuf_input(case)
    _aux_with_planes(ops.pixel_shuffle2, x.to(cuda), sb.pixshuf_ref(x))
