"""The premises of tests/test_gpu_se_block.py, checked on the CPU: that its cases and bars can tell a subtly wrong kernel
from a right one.  Each test states the wrong kernel it stands for."""
import pytest
import torch

import se_block_common as sb


@pytest.mark.parametrize("shape", sb.RS_SHAPES + sb.RS_S1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gates_tell_images_apart(shape):
    """(a) A kernel that gave a row its neighbour image's gates: the reference with the gates rolled by one image is at least
    100 bars away from the true one in EVERY row adjacent to an image boundary (in the row's worst channel), in both add orders
    and under both bars."""
    N, H, W, Cin, Cout, st, k = shape
    for rounded, fam in ((False, "f32"), (True, "f16")):
        if shape in sb.RS_S1_SHAPES and not rounded:
            continue                                            # (the streaming kernel is an f16 kernel)
        x, w, b, R, gates, y64 = sb.rs_problem(shape, rounded, sb.rs_seed(shape))
        hw = y64.shape[1] * y64.shape[2]
        rows = sb.boundary_rows(N, hw)
        assert len(rows) == 2 * (N - 1) and N >= 2
        for act, after in sb.RS_ORDERS:
            _, ref = sb.scaled_skip_ref(y64, R, gates, act, after)
            _, wrong = sb.scaled_skip_ref(y64, R, torch.roll(gates, 1, 0), act, after)
            ratio = ((wrong - ref).abs() / sb.elem_bar(ref, fam)).reshape(N * hw, Cout)
            worst = ratio[rows].max(dim=1).values
            assert float(worst.min()) >= 100.0, (fam, act, after, float(worst.min()))


def test_power_of_two_gates_are_distinct():
    """... and the bit-identity oracle's gates differ between neighbouring images in every channel and among any four consecutive
    channels (what one thread of the staged epilogue owns), and scale fp32 numbers exactly."""
    for shape in sb.RS_SHAPES + sb.RS_S1_SHAPES:
        N, Cout = shape[0], shape[4]
        y = sb.pow2_gates(N, Cout)
        assert bool((y[1:] != y[:-1]).all())
        for c in range(0, Cout - 3, 4):
            assert len(set(y[0, c:c + 4].tolist())) == 4
        r = torch.randn(N, Cout, generator=torch.Generator().manual_seed(1))
        assert torch.equal((r * y).double(), r.double() * y.double())


@pytest.mark.parametrize("shape,k", [(s, k) for s in sb.POOL_SHAPES for k in (1, 3)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "k%d" % v)
def test_slab_sums_tell_rows_apart(shape, k):
    """(b) A pooled epilogue that dropped the last valid row of a slab (a wrong `nvalid`): the slab sums move by at least 100 bars
    in every slab (in the slab's worst channel).  The bar of a slab sum is the sum of its rows' element bars."""
    for rounded, fam in ((False, "f32"), (True, "f16")):
        x, w, b, y64 = sb.pool_problem(shape, k, rounded, sb.pool_seed(shape, k))
        rows = y64.reshape(-1, y64.shape[-1])
        bar = sb.slab_sums(sb.elem_bar(rows, fam))
        moved = (sb.slab_sums(rows) - sb.slab_sums(rows, drop_last=True)).abs()
        worst = (moved / bar).max(dim=1).values
        assert float(worst.min()) >= 100.0, (fam, float(worst.min()))
    nv = sb.slab_rows(rows.shape[0])
    assert sum(nv) == rows.shape[0] and all(1 <= v <= 64 for v in nv)


def test_pool_cases_hold_the_edges():
    """... and the pool shapes hold a partial last slab, a Cout overhang in the last 64-wide N tile, exact slabs and a batch."""
    ms = [s[0] * s[1] * s[2] for s in sb.POOL_SHAPES]
    assert any(m % 64 for m in ms) and any(m % 64 == 0 for m in ms)
    assert any(s[4] % 64 for s in sb.POOL_SHAPES)
    assert any(s[0] > 1 and (s[1] * s[2]) % 64 == 0 for s in sb.POOL_SHAPES)
    assert any(p[3] == 3 for p in sb.pool_params()) and any(p[1] == 1 for p in sb.pool_params())


def test_avgpool_cases_hold_empty_and_short_slices():
    """(c) A kernel that read past HW in a short slice, or left an empty slice unwritten: the list holds both kinds."""
    empty = short = 0
    for HW in sb.AVGPOOL_HW:
        P = sb.avgpool_parts(HW)
        per, bounds = sb.slice_bounds(HW, P)
        assert per * P >= HW
        empty += any(lo >= HW for lo, hi in bounds)
        short += any(0 < hi - lo < per for lo, hi in bounds)
    assert empty >= 1 and short >= 1
    per, bounds = sb.slice_bounds(2050, sb.avgpool_parts(2050))
    assert (sb.avgpool_parts(2050), per) == (64, 33) and bounds[62] == (2046, 2050) and bounds[63][0] >= 2050
    # every size class of avgpool_parts, and both sides of each threshold
    assert {sb.avgpool_parts(h) for h in sb.AVGPOOL_HW} == {2, 8, 32, 64}
    # the slice sums of an empty slice are zeros, and the slices partition the pixels
    x = torch.randn(2, 2050, 3, generator=torch.Generator().manual_seed(2))
    s, _ = sb.slice_sums(x, 64)
    assert bool((s[:, 63] == 0).all()) and torch.allclose(s.sum(1), x.double().sum(1))
    N, HW, C, c0, ld = sb.AVGPOOL_VIEW
    assert ld > c0 + C and c0 > 0 and c0 % 4 == 0


def test_fc_cases_reach_every_staging_branch():
    """(d) A staging branch of fc_kernel that was wrong: the list reaches G = 4, G = 2, and G = 1 with and without slice sums, both
    sides of Cin <= 512 (four LDS copies of the vector, or one), and a Cout that is no multiple of the eight neurons of a block."""
    seen = {(sb.fc_staging_groups(c, p), p > 1) for c in sb.FC_CIN for p in sb.FC_PARTS}
    assert {(4, True), (2, True), (1, True), (1, False)} <= seen
    assert any(c <= 512 for c in sb.FC_CIN) and any(c > 512 for c in sb.FC_CIN)
    assert 512 in sb.FC_CIN and any(512 < c < 512 + 8 for c in sb.FC_CIN)       # the threshold itself and the first size past it
    assert any(c // 4 == 64 for c in sb.FC_CIN) and any(c // 4 == 65 for c in sb.FC_CIN)      # ... and of the G = 4 / G = 2 switch
    assert any(o % 8 for o in sb.FC_COUT) and 1 in sb.FC_COUT
    assert all(c % 4 == 0 for c in sb.FC_CIN)
    # the reference: slice sums are added and scaled, a plain vector is not scaled
    x = torch.randn(2, 3, 8, generator=torch.Generator().manual_seed(3))
    w, b = torch.randn(5, 8), torch.randn(5)
    assert torch.allclose(sb.fc_ref(x, w, b, "linear", 0.25), (0.25 * x.double().sum(1)) @ w.double().t() + b.double())
    assert torch.allclose(sb.fc_ref(x[:, :1], w, b, "linear", 0.25), sb.fc_ref(x[:, 0], w, b, "linear", 1.0))
    assert bool((sb.fc_ref(x, w, b, "relu", 1.0) >= 0).all()) and float(sb.fc_ref(x, w, b, "sigmoid", 1.0).max()) < 1.0


@pytest.mark.parametrize("case", sb.MAXPOOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_maxpool_inputs_are_negative(case):
    """(e) A max-pool that padded with 0 instead of -inf: more than 90 % of the inputs are negative, so the zero-padded result
    differs from the true one -- at every border output whose window has no positive element."""
    x = sb.maxpool_input(case)
    assert float((x < 0).float().mean()) > 0.9
    ref, wrong = sb.maxpool_ref(x), sb.maxpool_zero_padded(x)
    N, H, W, C = case
    assert ref.shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)      # the engine's output size is torch's
    assert float((ref != wrong).float().mean()) > 0.2
    assert bool((ref[:, 0] != wrong[:, 0]).any()) and bool((ref[:, :, 0] != wrong[:, :, 0]).any())


def test_pixel_shuffle_reference_is_the_kernel_comment():
    """out[c, 2h+i, 2w+j] = in[4c + 2i + j, h, w] (aux_kernels.hip), in NHWC."""
    x = sb.pixshuf_input(sb.PIXSHUF_CASES[0])
    ref = sb.pixshuf_ref(x)
    N, H, W, C = x.shape
    for (n, h, w_, c, i, j) in [(0, 0, 0, 0, 0, 0), (1, 2, 4, 1, 1, 0), (0, 1, 3, 1, 0, 1), (1, 2, 0, 0, 1, 1)]:
        assert float(ref[n, 2 * h + i, 2 * w_ + j, c]) == float(x[n, h, w_, 4 * c + 2 * i + j])


def test_case_lists_are_the_issue_s():
    """The launches that are made: every tile family per scaled-skip shape, three K slices reached on the staged path in both 16-bit
    families and in fp32, the element-wise fallback reached in every family, and the streaming kernel's four shapes eligible by size."""
    params = sb.rs_params()
    for shape in sb.RS_SHAPES:
        fams = {sb.family(t) for s, t, _ in params if s == shape}
        assert fams == {"f32", "b3", "f16"}
    staged3 = {sb.family(t) for s, t, sp in params if sp == 3 and s[4] % 4 == 0 and "halo" not in t}
    assert staged3 == {"f32", "b3", "f16"}
    elementwise = {sb.family(t) for s, t, _ in params if s[4] % 4 != 0}
    assert elementwise == {"f32", "b3", "f16"}
    assert any("halo" in t for _, t, _ in params)
    for N, H, W, Cin, Cout, st, k in sb.RS_S1_SHAPES:
        OH, OW = sb.out_hw(H, W, 1, st, 0)
        assert k == 1 and N * OH * OW >= 2048 and OH * OW >= 32 and Cout >= 128 and Cin in (64, 128, 256, 384, 512, 1024)
