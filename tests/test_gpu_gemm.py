"""GPU tests of the hand-written 1x1-convolution GEMM (gemm.hip): product, folded BatchNorm statistics, normalise-on-load
prologue, grouped form -- against plain torch f32 arithmetic on the same bf16 operands; at the end every form on every
tile configuration, and every weight-gradient tile, bit for bit against float64 on exact operands (tests/_gemm_ref.py).
`pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(torch.bfloat16).to(DEV)


def _check_product(y, ref):
    """bf16 result of an f32 accumulation in ANOTHER order: equal up to one rounding step on a small fraction."""
    y, ref = y.float(), ref.float()
    tol = ref.abs() * 2.0 ** -7 + ref.abs().max() * 2.0 ** -15
    bad = (y - ref).abs() > tol
    assert not bool(bad.any()), (int(bad.sum()), float((y - ref).abs().max()))
    assert float((y != ref).float().mean()) < 5e-3


# (R, K, groups, M, views): every stage shape of the encoder at a small batch, ragged ranges, R < tile, grouped
SHAPES = [(64, 64, 1, 8192, 2), (256, 64, 1, 8192, 2), (64, 256, 1, 8192, 2), (128, 128, 4, 4096, 2),
          (128, 64, 1, 2048 * 3, 1), (512, 2048, 1, 1024, 2), (2048, 512, 1, 1024, 1), (256, 768, 1, 2560, 2),
          (1024, 1024, 4, 2048, 2), (96, 32, 1, 1280, 1), (64, 64, 1, 128 * 2 * 37, 2),
          # the 512-column tiles of round 3 (<= 128 rows per group, >= 2^16 columns per view): N64, N32 (grouped: one
          # chunk per tile), N128, N128 with ragged rows, N64 with a ragged last column range, one-view N32
          (64, 256, 1, 131072, 2), (128, 128, 4, 131072, 2), (128, 512, 1, 262144, 2), (96, 160, 1, 524288, 1),
          (64, 64, 1, 2 * 512 * 131, 2), (32, 96, 1, 65536, 1),
          # the four-wave 256 x 256 tile of round 4 (gemm_xl.h: 256 / 512 rows, >= 512 operand rows, ungrouped): ragged
          # column ranges, one tile per workgroup, one view, a deep contraction
          (256, 512, 1, 2 * 256 * 9, 2), (512, 1280, 1, 256 * 7, 1), (512, 512, 1, 256, 1), (256, 2560, 1, 2 * 256 * 33, 2)]


def _plan_cfg(R, K, groups, M, views):
    import ctypes
    from grafp_amd._lib import lib
    info = (ctypes.c_int * 8)()
    assert lib.grafp_conv1x1_gemm_plan(R, K, groups, M, views, info) == 0
    return info[0]


def test_the_four_wave_tile_is_what_these_shapes_run_on():
    """The shapes above that are meant for the four-wave tile (plan code 5) do take it, the others do not: 1024+ output
    rows, K < 512 and grouped products stay on the eight-wave tile (measured: profiles/r04_gemm_xl_2048.txt)."""
    for shape in ((256, 512, 1, 2 * 256 * 9, 2), (512, 1280, 1, 256 * 7, 1), (512, 512, 1, 256, 1), (512, 2048, 1, 1024, 2),
                  (256, 768, 1, 2560, 2), (256, 2560, 1, 2 * 256 * 33, 2), (512, 1024, 1, 262144, 2)):
        assert _plan_cfg(*shape) == 5, shape
    for shape in ((2048, 512, 1, 1024, 1), (1024, 256, 1, 524288, 2), (1024, 1024, 4, 2048, 2), (256, 256, 1, 524288, 2),
                  (64, 256, 1, 8192, 2)):
        assert _plan_cfg(*shape) != 5, shape


@pytest.mark.parametrize("R,K,M", [(256, 512, 256 * 12), (512, 1536, 256 * 6)])
def test_four_wave_tile_launches_are_bit_identical_and_leave_no_trace_of_the_ring(R, K, M):
    """The tile prefetches fragments across its chunk barrier and spreads a tile's epilogue over the next tile's chunks:
    a misplaced wait shows up as run-to-run differences.  16 launches each of the plain, the statistics and the
    concatenated-operand form on NaN-poisoned outputs: identical bits, every element written."""
    from grafp_amd import ops
    assert _plan_cfg(R, K, 1, M, 2) == 5
    w, x = _rand((R, K), 11, 0.2), _rand((K, M), 12, 1.0, 0.3)
    x1, x2 = x[:K - 256].contiguous(), x[K - 256:].contiguous()
    first = None
    for rep in range(16):
        junk = torch.full((R, M), float("nan"), dtype=torch.bfloat16, device=DEV)
        del junk
        y, part = ops.conv1x1_gemm(w, x, 1, 2, stats=True)
        yp = ops.conv1x1_gemm(w, x, 1, 2)
        yc = ops.conv1x1_gemm_cat(w, x1, x2)
        assert not bool(torch.isnan(y.float()).any())
        got = (y.clone(), part.clone(), yp.clone(), yc.clone())
        if first is None:
            first = got
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, got)), rep
    assert torch.equal(first[0], first[2]) and torch.equal(first[0], first[3])
    ref = (w.float() @ x.float()).to(torch.bfloat16)
    _check_product(first[0], ref)


@pytest.mark.parametrize("R,K,groups,M,views", SHAPES)
def test_gemm_product_and_stats(R, K, groups, M, views):
    from grafp_amd import ops
    assert ops.gemm_supported(R, K, groups, M, views)
    w = _rand((R, K // groups), 1, 0.2)
    x = _rand((K, M), 2, 1.0, 0.3)
    y, part = ops.conv1x1_gemm(w, x, groups, views, stats=True)
    y2 = ops.conv1x1_gemm(w, x, groups, views)
    assert torch.equal(y, y2)                       # the statistics epilogue does not change the product
    wf, xf = w.float(), x.float()
    Rg, Kg = R // groups, K // groups
    ref = torch.cat([wf[g * Rg:(g + 1) * Rg] @ xf[g * Kg:(g + 1) * Kg] for g in range(groups)], dim=0)
    _check_product(y, ref.to(torch.bfloat16))
    # statistics of the ROUNDED outputs, per view
    gamma = torch.linspace(0.5, 1.5, R, device=DEV)
    beta = torch.linspace(-0.2, 0.2, R, device=DEV)
    bias = torch.linspace(-1.0, 1.0, R, device=DEV)
    rm, rv = torch.zeros(R, device=DEV), torch.ones(R, device=DEV)
    mean, invstd, tab = ops.bn_finalize(part, R, K, groups, M, views, gamma, beta, bias, rm, rv, True, 0.1, 1e-5)
    yv = y.float().reshape(R, views, M // views).double()
    want_mean = yv.mean(dim=2) + bias.double()[:, None]
    want_var = yv.var(dim=2, unbiased=False)
    np.testing.assert_allclose(mean.cpu().numpy(), want_mean.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(invstd.cpu().numpy(), (1.0 / torch.sqrt(want_var + 1e-5)).cpu().numpy(), rtol=2e-5)
    scale = gamma.double()[:, None] * (1.0 / torch.sqrt(want_var + 1e-5))
    np.testing.assert_allclose(tab[..., 0].cpu().numpy(), scale.cpu().numpy(), rtol=2e-5)
    np.testing.assert_allclose(tab[..., 1].cpu().numpy(), (beta.double()[:, None] - yv.mean(dim=2) * scale).cpu().numpy(),
                               rtol=1e-4, atol=1e-4)
    # running statistics: once per view, in order, unbiased variance
    erm, erv = torch.zeros(R, dtype=torch.float64, device=DEV), torch.ones(R, dtype=torch.float64, device=DEV)
    for v in range(views):
        erm = 0.9 * erm + 0.1 * want_mean[:, v]
        erv = 0.9 * erv + 0.1 * yv[:, v].var(dim=1, unbiased=True)
    np.testing.assert_allclose(rm.cpu().numpy(), erm.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rv.cpu().numpy(), erv.cpu().numpy(), rtol=1e-5)
    # the apply half
    res = _rand((R, M), 5)
    z = ops.bn_affine(y, tab, views, residual=res, act=ops.ACT_RELU)
    t = tab.reshape(R, views, 1, 2)
    zr = torch.relu(torch.addcmul(t[..., 1], y.float().reshape(R, views, -1), t[..., 0])).reshape(R, M) + res.float()
    assert float((z.float() - zr.to(torch.bfloat16).float()).abs().max()) <= float(zr.abs().max()) * 2.0 ** -7
    # finalize + affine as ONE launch: the same bits everywhere
    if views <= 4:
        rm2, rv2 = torch.zeros(R, device=DEV), torch.ones(R, device=DEV)
        z2, mean2, invstd2, tab2 = ops.bn_finalize_affine(y, part, K, groups, views, gamma, beta, bias, rm2, rv2, 0.1, 1e-5,
                                                          residual=res, act=ops.ACT_RELU)
        assert torch.equal(z2, z) and torch.equal(mean2, mean) and torch.equal(invstd2, invstd) and torch.equal(tab2, tab)
        assert torch.equal(rm2, rm) and torch.equal(rv2, rv)


def test_gemm_statistics_with_large_mean():
    """|mean| >> std rows: the shifted sums keep the variance (E[y^2] - E[y]^2 in f32 would lose it)."""
    from grafp_amd import ops
    R, K, M = 64, 64, 128 * 64
    w = torch.zeros((R, K), dtype=torch.bfloat16, device=DEV)
    w[:, 0] = 1.0
    w[torch.arange(R), 1 + torch.arange(R) % (K - 1)] = 0.01
    x = _rand((K, M), 3)
    x[0] = 200.0
    y, part = ops.conv1x1_gemm(w, x, 1, 1, stats=True)
    one = torch.ones(R, device=DEV)
    mean, invstd, _ = ops.bn_finalize(part, R, K, 1, M, 1, one, 0 * one, None, None, None, True, 0.1, 0.0)
    yv = y.float().double()
    np.testing.assert_allclose(mean[:, 0].cpu().numpy(), yv.mean(dim=1).cpu().numpy(), rtol=1e-6)
    np.testing.assert_allclose(invstd[:, 0].cpu().numpy(), (1 / yv.std(dim=1, unbiased=False)).cpu().numpy(), rtol=1e-4)


def _plan_info(R, K, groups, M, views):
    import ctypes
    from grafp_amd._lib import lib
    info = (ctypes.c_int * 8)()
    assert lib.grafp_conv1x1_gemm_plan(R, K, groups, M, views, info) == 0
    return list(info)


# ((R, K, groups, M, views), tile configuration): per configuration the smallest shape the plan rule sends there -- S, L,
# XL, N32, N64, N128 -- and an N64 shape whose last column range is short (131 tiles in ranges of 4)
PART_SHAPES = [((64, 64, 1, 256, 2), 0), ((512, 64, 1, 512, 1), 1), ((256, 512, 1, 512, 2), 5), ((32, 32, 1, 65536, 1), 2),
               ((64, 64, 1, 65536, 1), 3), ((128, 512, 1, 131072, 1), 4), ((64, 64, 1, 2 * 512 * 131, 2), 3)]


@pytest.mark.parametrize("shape,cfg", PART_SHAPES)
def test_gemm_partials_against_float64(shape, cfg):
    """The layout of the statistics partials, which the end of a STATS kernel writes and the finalizers read: part[r][v][p]
    = (0, M2, mean) of row r over the columns of range p of view v (info[2] tiles of info[6] columns, the last range of a
    view what is left), against float64 on the rounded y.  mean: the bar of test_gemm_product_and_stats; M2: rtol 4e-5,
    twice that test's bar on invstd (invstd ~ var^-1/2)."""
    from grafp_amd import ops
    R, K, groups, M, views = shape
    info = _plan_info(*shape)
    assert info[0] == cfg == _plan_cfg(*shape)
    w, x = _rand((R, K // groups), 1, 0.2), _rand((K, M), 2, 1.0, 0.3)
    y, part = ops.conv1x1_gemm(w, x, groups, views, stats=True)
    Mg, cols, P = M // views, info[2] * info[6], info[3]
    assert part.shape == (R, views, P, 3) and P == -(-Mg // cols)
    yv = y.float().double().reshape(R, views, Mg)
    full = Mg // cols
    segs = [yv[:, :, :full * cols].reshape(R, views, full, cols)] + ([yv[:, :, full * cols:, None].transpose(2, 3)] if P > full else [])
    mean = torch.cat([s.mean(dim=3) for s in segs], dim=2)
    m2 = torch.cat([((s - s.mean(dim=3, keepdim=True)) ** 2).sum(dim=3) for s in segs], dim=2)
    got = part.double()
    print(f"{shape}: cfg {cfg}, {P} ranges of {cols} columns (last {Mg - (P - 1) * cols}); worst deviation: mean "
          f"{float((got[..., 2] - mean).abs().max()):.3e} abs, M2 {float(((got[..., 1] - m2).abs() / m2).max()):.3e} rel")
    assert bool((part[..., 0] == 0).all())
    np.testing.assert_allclose(got[..., 2].cpu().numpy(), mean.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[..., 1].cpu().numpy(), m2.cpu().numpy(), rtol=4e-5)


def test_bn_finalize_in_eval_mode():
    """bn_finalize(training=False): mean, invstd and the (scale, shift) table from the RUNNING statistics (the conv bias
    goes into the shift only), the same for every view, against the float64 formula within the bars of
    test_gemm_product_and_stats; the running statistics stay as they are."""
    from grafp_amd import ops
    R, K, groups, M, views, eps = 64, 64, 1, 256, 2, 1e-5
    g = torch.Generator().manual_seed(7)
    gamma, beta = torch.linspace(0.5, 1.5, R, device=DEV), torch.linspace(-0.2, 0.2, R, device=DEV)
    bias = torch.linspace(-1.0, 1.0, R, device=DEV)
    rm, rv = torch.randn(R, generator=g).to(DEV), (torch.rand(R, generator=g) + 0.1).to(DEV)
    rm0, rv0 = rm.clone(), rv.clone()
    mean, invstd, tab = ops.bn_finalize(None, R, K, groups, M, views, gamma, beta, bias, rm, rv, False, 0.1, eps)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    want_invstd = 1.0 / torch.sqrt(rv0.double() + eps)
    scale = gamma.double() * want_invstd
    shift = beta.double() + (bias.double() - rm0.double()) * scale
    for v in range(views):
        np.testing.assert_allclose(mean[:, v].cpu().numpy(), rm0.double().cpu().numpy(), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(invstd[:, v].cpu().numpy(), want_invstd.cpu().numpy(), rtol=2e-5)
        np.testing.assert_allclose(tab[:, v, 0].cpu().numpy(), scale.cpu().numpy(), rtol=2e-5)
        np.testing.assert_allclose(tab[:, v, 1].cpu().numpy(), shift.cpu().numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("R,K,groups,M,views,act", [(64, 128, 1, 4096, 2, 1), (128, 256, 1, 2048, 2, 1),
                                                    (64, 128, 1, 131072, 2, 1), (128, 512, 1, 131072, 1, 2),
                                                    (512, 2048, 1, 1024, 2, 1), (64, 64, 1, 2048, 1, 2),
                                                    (128, 128, 4, 2048, 2, 0)])
def test_gemm_normalise_on_load(R, K, groups, M, views, act):
    from grafp_amd import ops
    w = _rand((R, K // groups), 11, 0.2)
    x = _rand((K, M), 12, 2.0, 1.0)
    g = torch.Generator().manual_seed(13)
    tab = torch.stack((torch.rand((K, views), generator=g) + 0.5, torch.randn((K, views), generator=g)), dim=-1).to(DEV)
    y, part = ops.conv1x1_gemm(w, x, groups, views, pro_tab=tab, pro_act=act, pro_slope=0.2, stats=True)
    t = tab.reshape(K, views, 1, 2)
    u = torch.addcmul(t[..., 1], x.float().reshape(K, views, -1), t[..., 0])          # fma rounding differs by <= 1 ulp f32
    u = torch.relu(u) if act == 1 else (torch.where(u > 0, u, 0.2 * u) if act == 2 else u)
    u = u.reshape(K, M).to(torch.bfloat16).float()
    Rg, Kg = R // groups, K // groups
    ref = torch.cat([w.float()[i * Rg:(i + 1) * Rg] @ u[i * Kg:(i + 1) * Kg] for i in range(groups)], dim=0)
    y, ref = y.float(), ref.to(torch.bfloat16).float()
    # an f32 fma vs mul+add can move an operand across a bf16 rounding boundary (rare): bound the relative L2 error too
    assert float((y - ref).norm() / ref.norm()) < 2e-3
    assert float(((y - ref).abs() > ref.abs() * 2.0 ** -6 + ref.abs().max() * 2.0 ** -12).float().mean()) < 1e-3


@pytest.mark.parametrize("R,K,M,views", [(64, 128, 1 << 21, 2), (64, 256, 1 << 21, 2), (128, 256, 1 << 20, 2),
                                         (128, 512, 1 << 20, 2), (64, 128, 1 << 14, 2)])
def test_normalise_on_load_is_bitwise_the_separate_pass_at_training_sizes(R, K, M, views):
    """The stage 0-1 consumers of a 1024-pair step (2048 clip-views) and a small one: the product with the operand
    normalised in the fragment registers equals bn_affine + plain product BIT FOR BIT, run after run, and the weight
    gradient with the same transform equals the plain one on the materialised operand up to its summation order.
    (The round 1-3 form -- an in-place pass over the staged LDS tile -- raced with the LDS-DMA ring on the two-workgroup
    tile at exactly these sizes: 0.6 % of the outputs wrong, different from run to run; the small shapes never showed it.)"""
    from grafp_amd import ops
    g = torch.Generator().manual_seed(R + K)
    x = torch.randn(K, M, generator=g).to(torch.bfloat16).to(DEV)
    go = torch.randn(R, M, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(R, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    tab = torch.stack((torch.rand(K, views, generator=g) + 0.5, torch.randn(K, views, generator=g)), dim=-1).contiguous().to(DEV)
    z = ops.bn_affine(x, tab, views, None, ops.ACT_RELU)
    y0, p0 = ops.conv1x1_gemm(w, z, 1, views, stats=True)
    d0 = ops._wgrad_bf16(go, z, R, K, 1, M)
    for _ in range(3):
        y1, p1 = ops.conv1x1_gemm(w, x, 1, views, pro_tab=tab, pro_act=ops.ACT_RELU, stats=True)
        assert torch.equal(y1, y0)
        one = torch.ones(R, device=DEV)
        m0 = ops.bn_finalize(p0, R, K, 1, M, views, one, 0 * one, None, None, None, True, 0.1, 1e-5)
        m1 = ops.bn_finalize(p1, R, K, 1, M, views, one, 0 * one, None, None, None, True, 0.1, 1e-5)
        assert all(torch.equal(a_, b_) for a_, b_ in zip(m0, m1))        # identical outputs, identical statistics
        d1 = ops._wgrad_bf16(go, x, R, K, 1, M, views, tab, ops.ACT_RELU, 0.0)
        assert float((d1 - d0).norm() / d0.norm()) <= 2e-6


@pytest.mark.parametrize("R,K,M,views,groups", [(64, 128, 1 << 21, 2, 1), (64, 256, 1 << 20, 2, 1), (128, 128, 1 << 21, 2, 2)])
def test_statistics_epilogue_is_deterministic_from_launch_to_launch(R, K, M, views, groups):
    """Ten launches on the same operands: identical outputs AND identical statistics partials.  (Round 3: with 64-row wave
    tiles the partials of rows 48-63 of a few workgroups differed from launch to launch -- one accumulate of lanes 48-63 took
    0 instead of the shift when hipcc splatted the shift by operand selection from a register pair shared by two row tiles;
    the kernel now keeps the shift in a register pair of its own.  y was always identical, the statistics were off by 1e-6.)"""
    from grafp_amd import ops
    g = torch.Generator().manual_seed(R * 7 + K)
    x = torch.randn(K, M, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(R, K // groups, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    one = torch.ones(R, device=DEV)
    ref = None
    for _ in range(10):
        y, p = ops.conv1x1_gemm(w, x, groups, views, stats=True)
        m = ops.bn_finalize(p, R, K, groups, M, views, one, 0 * one, None, None, None, True, 0.1, 1e-5)
        cur = (y, m[0], m[1], m[2])
        if ref is None:
            ref = tuple(t_.clone() for t_ in cur)
        else:
            assert all(torch.equal(a, b) for a, b in zip(ref, cur))


def test_gemm_rejects_unsupported_shapes():
    from grafp_amd import ops
    assert not ops.gemm_supported(64, 8, 1, 1024, 1)        # K = 8 (the stem): library GEMM
    assert not ops.gemm_supported(64, 64, 1, 1000, 1)
    w, x = _rand((64, 8), 1), _rand((8, 1024), 2)
    with pytest.raises(RuntimeError):
        ops.conv1x1_gemm(w, x)


# (cout, cin, groups, M, views): the three tile configurations (64 / 128 / 256), grouped, ragged rows, short slices
WG_SHAPES = [(64, 64, 1, 8192, 2), (256, 64, 1, 16384, 2), (128, 128, 4, 8192, 2), (128, 256, 1, 4096, 1),
             (1024, 256, 1, 2048, 2), (512, 2048, 1, 1024, 2), (96, 160, 1, 1280, 1), (64, 256, 1, 262144, 2),
             # >= 2^19 columns: the rule picks the 256-byte-piece tile (T128) for the small outputs, grouped ones included
             (64, 128, 1, 524288, 2), (128, 128, 4, 524288, 1),
             # ... and the 128 x 128 tile on 256-byte pieces (S128) from 250 MB of operands
             (128, 256, 1, 524288, 1)]


@pytest.mark.parametrize("cout,cin,groups,M,views", WG_SHAPES)
@pytest.mark.parametrize("pro", [False, True])
def test_wgrad_dma(cout, cin, groups, M, views, pro):
    """LDS-DMA weight gradient (plain and with the normalise-on-load X operand) vs a float64 product of the same bf16
    operands: 2e-3 of the largest entry."""
    from grafp_amd import ops
    g = _rand((cout, M), 21)
    x = _rand((cin, M), 22, 1.5, 0.5)
    tab = None
    xe = x.float()
    if pro:
        gen = torch.Generator().manual_seed(23)
        tab = torch.stack((torch.rand((cin, views), generator=gen) + 0.5, torch.randn((cin, views), generator=gen)), -1).to(DEV)
        t = tab.reshape(cin, views, 1, 2)
        xe = torch.relu(torch.addcmul(t[..., 1], x.float().reshape(cin, views, -1), t[..., 0])).reshape(cin, M)
        xe = xe.to(torch.bfloat16).float()
    dw = ops.conv1x1_wgrad(g, x, cout, cin, groups, M, views, tab, ops.ACT_RELU if pro else ops.ACT_NONE)
    gd, xd = g.double(), xe.double()
    og, cg = cout // groups, cin // groups
    want = torch.cat([gd[i * og:(i + 1) * og] @ xd[i * cg:(i + 1) * cg].t() for i in range(groups)], dim=0)
    assert dw.shape == (cout, cg) and dw.dtype == torch.float32
    tol = (4e-3 if pro else 2e-3) * float(want.abs().max())      # pro: an f32 fma can flip an operand's bf16 rounding
    assert float((dw.double() - want).abs().max()) <= tol
    # deterministic (fixed-order reduction, no atomics)
    assert torch.equal(dw, ops.conv1x1_wgrad(g, x, cout, cin, groups, M, views, tab, ops.ACT_RELU if pro else ops.ACT_NONE))


# T, S, L (128-byte pieces), S32, M32, L32 (64-byte pieces), SG, LG (G through registers), T128, S128 (256-byte pieces)
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7, 8, 10])
@pytest.mark.parametrize("cout,cin,groups,M,views", [(256, 64, 1, 16384, 2), (1024, 256, 1, 2048, 2), (512, 1024, 4, 1024, 2),
                                                     (96, 160, 1, 1280, 1), (256, 512, 1, 64, 1), (320, 256, 1, 4160, 1)])
def test_wgrad_every_tile_configuration(tile, cout, cin, groups, M, views):
    """The heuristic picks the wide configurations only at sizes a test cannot afford for every shape: force each one
    (the `tile` argument of grafp_conv1x1_wgrad_tile_bf16) on small cases -- ragged rows, one chunk per slice, odd chunk counts, groups."""
    from grafp_amd import ops
    g, x = _rand((cout, M), 31), _rand((cin, M), 32, 1.5, 0.5)
    dw = ops.conv1x1_wgrad(g, x, cout, cin, groups, M, views, tile=tile)
    again = ops.conv1x1_wgrad(g, x, cout, cin, groups, M, views, tile=tile)
    og, cg = cout // groups, cin // groups
    want = torch.cat([g[i * og:(i + 1) * og].double() @ x[i * cg:(i + 1) * cg].double().t() for i in range(groups)], dim=0)
    assert float((dw.double() - want).abs().max()) <= 2e-3 * float(want.abs().max())
    assert torch.equal(dw, again)


# ragged rows; groups and views; one chunk per slice (T128 and S128 fall back to T and S)
WG_PRO_SHAPES = [(96, 160, 1, 1280, 1), (512, 1024, 4, 1024, 2), (256, 512, 1, 64, 1)]
_WG_PRO_CASES = {}


def _wg_pro_case(shape):
    """(g, x, ReLU pro_tab, float64 product of the bf16-rounded transformed operand) of a shape, made once."""
    if shape not in _WG_PRO_CASES:
        cout, cin, groups, M, views = shape
        g, x = _rand((cout, M), 21), _rand((cin, M), 22, 1.5, 0.5)
        gen = torch.Generator().manual_seed(23)
        tab = torch.stack((torch.rand((cin, views), generator=gen) + 0.5, torch.randn((cin, views), generator=gen)), -1).to(DEV)
        t = tab.reshape(cin, views, 1, 2)
        xe = torch.relu(torch.addcmul(t[..., 1], x.float().reshape(cin, views, -1), t[..., 0])).reshape(cin, M)
        gd, xd = g.double(), xe.to(torch.bfloat16).double()
        og, cg = cout // groups, cin // groups
        want = torch.cat([gd[i * og:(i + 1) * og] @ xd[i * cg:(i + 1) * cg].t() for i in range(groups)], dim=0)
        _WG_PRO_CASES[shape] = (g, x, tab, want)
    return _WG_PRO_CASES[shape]


# T, S, L, S32, M32, L32, T128, S128: every configuration that has the normalise-on-load form
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 8, 10])
@pytest.mark.parametrize("shape", WG_PRO_SHAPES)
def test_wgrad_every_dma_tile_with_normalise_on_load(tile, shape):
    """The rule picks three tiles with a pro_tab; the other five are reachable through `tile` only.  Reference and bar
    of test_wgrad_dma."""
    from grafp_amd import ops
    cout, cin, groups, M, views = shape
    g, x, tab, want = _wg_pro_case(shape)
    dw = ops.conv1x1_wgrad(g, x, cout, cin, groups, M, views, tab, ops.ACT_RELU, tile=tile)
    assert dw.shape == (cout, cin // groups) and dw.dtype == torch.float32
    assert float((dw.double() - want).abs().max()) <= 4e-3 * float(want.abs().max())
    assert torch.equal(dw, ops.conv1x1_wgrad(g, x, cout, cin, groups, M, views, tab, ops.ACT_RELU, tile=tile))


@pytest.mark.parametrize("tile", [6, 7])
@pytest.mark.parametrize("shape", WG_PRO_SHAPES)
def test_wgrad_forced_register_staged_g_is_ignored_with_normalise_on_load(tile, shape):
    """SG and LG have no normalise-on-load form: with a pro_tab the rule's own choice runs, bit for bit."""
    from grafp_amd import ops
    cout, cin, groups, M, views = shape
    g, x, tab, _ = _wg_pro_case(shape)
    dw = ops.conv1x1_wgrad(g, x, cout, cin, groups, M, views, tab, ops.ACT_RELU, tile=tile)
    assert torch.equal(dw, ops.conv1x1_wgrad(g, x, cout, cin, groups, M, views, tab, ops.ACT_RELU, tile=-1))


@pytest.mark.parametrize("cout,cin,groups,M,views", [(64, 64, 1, 8192, 2), (1024, 256, 1, 2048, 2), (40, 24, 1, 777, 1)])
def test_wgrad_partials_report_the_slices_of_the_plan_query(cout, cin, groups, M, views):
    """n_slices of grafp_conv1x1_wgrad_partials_bf16 = info[3] of grafp_conv1x1_wgrad_plan, on LDS-DMA shapes and on one
    the register-staged kernel takes (info[0] == -1)."""
    import ctypes
    from grafp_amd import ops
    from grafp_amd._lib import lib
    info = (ctypes.c_int * 8)()
    assert lib.grafp_conv1x1_wgrad_plan(cout, cin, groups, M, views, info) == 0
    assert (info[0] == -1) == (cout == 40)
    g, x = _rand((cout, M), 31), _rand((cin, M), 32, 1.5, 0.5)
    nbytes = lib.grafp_conv1x1_wgrad_tile_workspace(cout, cin, groups, M, views, -1)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    S = ctypes.c_int(0)
    ops.check(lib.grafp_conv1x1_wgrad_partials_bf16(ops._p(g), ops._p(x), cout, cin, groups, M, views, None, 0, 0.0, -1,
                                                    ops._p(ws), nbytes, ctypes.byref(S), ops._stream()), "conv1x1_wgrad_partials")
    torch.cuda.synchronize()
    assert S.value == info[3] and S.value * cout * (cin // groups) * 4 <= nbytes


def test_gemm_cat_equals_product_plus_shortcut():
    """conv1x1_gemm_cat(W | I, dY, dZ) = W dY + dZ with ONE rounding (the data gradient of a residual block's first
    layer with the shortcut's gradient as extra operand rows), for an S-tile and an L-tile shape."""
    from grafp_amd import ops
    for R, K1, M in ((64, 64, 4096), (256, 1024, 2048), (128, 128, 1024), (64, 256, 65536), (128, 384, 131072 + 512)):
        wt = _rand((R, K1), 41, 0.1)
        dy, dz = _rand((K1, M), 42), _rand((R, M), 43)
        w_aug = torch.cat((wt, torch.eye(R, dtype=torch.bfloat16, device=DEV)), dim=1)
        got = ops.conv1x1_gemm_cat(w_aug, dy, dz)
        want = wt.double() @ dy.double() + dz.double()
        err = (got.double() - want).abs()
        assert float((err / (want.abs() + 1.0)).max()) <= 2.0 ** -8          # one bf16 rounding of an exact-ish f32 sum
        # and it is the concatenated product, bit for bit
        assert torch.equal(got, ops.conv1x1_gemm(w_aug, torch.cat((dy, dz), dim=0)))


def test_weights_prepare_one_launch():
    """ops.lowp_weights: bf16 copies, per-group transposed copies and [W^T | I] of many 1x1 convolutions in one launch
    == weight.to(bfloat16), its (grouped) transpose, and the concatenation with the identity."""
    from grafp_amd import ops
    torch.manual_seed(5)
    convs = [torch.nn.Conv2d(64, 256, 1, bias=False), torch.nn.Conv2d(128, 128, 1, groups=4), torch.nn.Conv2d(256, 64, 1),
             torch.nn.Conv2d(8, 64, 1, bias=False), torch.nn.Conv2d(96, 160, 1)]
    convs = [c.to(DEV) for c in convs]
    convs[0]._shortcut_first = True
    lw = ops.lowp_weights(convs)
    for rep in range(2):                                   # second pass: weights changed in place, same buffers
        if rep:
            with torch.no_grad():
                for c in convs:
                    c.weight.mul_(1.5).add_(0.01)
        lw.refresh(torch.bfloat16)
        for c in convs:
            want = c.weight.detach().to(torch.bfloat16)
            assert torch.equal(c._prepared.lowp.reshape(want.shape), want)
            R, Kg = want.shape[0], want.shape[1]
            if Kg % 32 or (R // c.groups) % 32:
                continue                                   # the 8-channel stem: plain cast only
            if getattr(c, "_shortcut_first", False):
                eye = torch.eye(Kg, dtype=torch.bfloat16, device=DEV)
                assert c._prepared.t is None and torch.equal(c._prepared.aug, torch.cat((want.reshape(R, Kg).t(), eye), dim=1))
            else:
                assert c._prepared.aug is None and torch.equal(c._prepared.t, ops._group_transpose(want.reshape(R, Kg), c.groups))


@pytest.mark.parametrize("R,K,groups,M,views,act", [(64, 64, 1, 8192, 2, 0), (256, 64, 1, 8192, 1, 1), (128, 128, 4, 4096, 2, 1),
                                                    (1024, 256, 1, 2048, 1, 1), (64, 256, 1, 131072, 2, 2),
                                                    (128, 512, 1, 262144, 1, 1), (96, 32, 1, 1280, 1, 1)])
def test_gemm_affine_epilogue_equals_gemm_plus_affine(R, K, groups, M, views, act):
    """Inference: z = act(bf16(W x) * scale + shift) formed in the GEMM's epilogue is bit-identical to the GEMM followed
    by the normalise pass (every tile configuration, grouped, ragged rows, both activations, per-view tables)."""
    from grafp_amd import ops
    w = _rand((R, K // groups), 51, 0.2)
    x = _rand((K, M), 52, 1.0, 0.3)
    g = torch.Generator().manual_seed(53)
    tab = torch.stack((torch.rand((R, views), generator=g) + 0.5, torch.randn((R, views), generator=g)), dim=-1).to(DEV)
    want = ops.bn_affine(ops.conv1x1_gemm(w, x, groups, views), tab, views, act=act, slope=0.2)
    got = ops.conv1x1_gemm_affine(w, x, tab, groups, views, act=act, slope=0.2)
    assert torch.equal(got, want)


def test_deferred_weight_gradient_reductions_are_bit_identical():
    """ops.defer_wgrad_reduce(): inside the block the weight gradients run only their split-K kernels, and the partial sums
    of ALL layers are reduced by one launch at its end (grafp_wgrad_reduce_multi; > 64 layers: two launches) -- the same
    summation tree as the per-layer reduction, so the same bits; a flush in the middle (what GradSync does when a bucket is
    complete) reduces what is queued so far; nested blocks reduce once, at the outer end."""
    from grafp_amd import ops
    shapes = [(64, 64, 1, 8192), (128, 128, 4, 4096), (256, 64, 1, 16384), (1024, 256, 1, 2048), (512, 512, 4, 1024),
              (64, 256, 1, 8192), (96, 32, 1, 1280)]
    ops_in = [(_rand((co, M), 20 + i), _rand((ci, M), 40 + i), co, ci, g, M) for i, (co, ci, g, M) in enumerate(shapes)]
    want = [ops.conv1x1_wgrad(G, X, co, ci, g, M).clone() for G, X, co, ci, g, M in ops_in]
    with ops.defer_wgrad_reduce():
        got = []
        for rep in range(10):                                   # 70 queued layers: more than one table
            for G, X, co, ci, g, M in ops_in:
                got.append(ops.conv1x1_wgrad(G, X, co, ci, g, M))
        with ops.defer_wgrad_reduce():                          # nested: still queued
            inner = ops.conv1x1_wgrad(*ops_in[0])
        assert len(ops._WGRAD_PENDING) == 71
    assert ops._WGRAD_PENDING is None
    for i, dw in enumerate(got):
        assert torch.equal(dw, want[i % len(shapes)]), i
    assert torch.equal(inner, want[0])
    with ops.defer_wgrad_reduce():
        a = ops.conv1x1_wgrad(*ops_in[1])
        ops.flush_wgrad_reduce()                                # a reader in the middle of backward
        assert torch.equal(a, want[1]) and ops._WGRAD_PENDING == []
        b = ops.conv1x1_wgrad(*ops_in[2])
    assert torch.equal(b, want[2])


def test_deferred_reduction_only_when_nothing_can_read_the_gradient_first():
    """under ops.defer_wgrad_reduce() a layer's dW leaves backward() unreduced only if autograd will ASSIGN it to a
    leaf weight's empty .grad.  A second backward pass without zeroing in between (gradient accumulation: AccumulateGrad
    ADDS into the existing .grad) and a tensor hook on the weight (it receives the gradient inside backward) must both see
    reduced values: those layers reduce immediately.  The layer is conv_bn_act on bf16 rows, as the encoder calls it."""
    from grafp_amd import ops
    R, K, M = 128, 64, 8192
    x = _rand((K, M), 61, 1.0, 0.2)
    gamma, beta = torch.ones(R, device=DEV), torch.zeros(R, device=DEV)
    up = _rand((R, M), 62).float()

    def backward(w, hook=None):
        rm, rv = torch.zeros(R, device=DEV), torch.ones(R, device=DEV)
        if hook is not None:
            w.register_hook(hook)
        z = ops.conv_bn_act(x, w, gamma, beta, rm, rv, True, act=ops.ACT_RELU)
        with ops.defer_wgrad_reduce():
            queued_inside = None
            (z.float() * up).sum().backward()
            queued_inside = len(ops._WGRAD_PENDING)
        return queued_inside

    w0 = (0.2 * torch.randn(R, K, generator=torch.Generator().manual_seed(63))).to(DEV)
    w = w0.clone().requires_grad_(True)
    assert backward(w) == 1                                   # the plain case IS deferred (one queued reduction)
    once = w.grad.clone()
    assert backward(w) == 0                                   # .grad exists: reduced immediately, then accumulated
    assert torch.equal(w.grad, once + once)
    seen = []
    w2 = w0.clone().requires_grad_(True)
    assert backward(w2, hook=lambda g: seen.append(g.clone())) == 0
    assert torch.equal(seen[0], once) and torch.equal(w2.grad, once)
    # a post-accumulate hook that is not GradSync's reads .grad inside backward -> reduced immediately
    seen_post = []
    w3 = w0.clone().requires_grad_(True)
    w3.register_post_accumulate_grad_hook(lambda p: seen_post.append(p.grad.clone()))
    assert backward(w3) == 0
    assert torch.equal(seen_post[0], once) and torch.equal(w3.grad, once)
    # ... and ONE weight used by two layers of the same pass: autograd adds the two gradients in front of AccumulateGrad,
    # so the second use reduces at once and flushes the first
    w4 = w0.clone().requires_grad_(True)
    rm, rv = torch.zeros(R, device=DEV), torch.ones(R, device=DEV)
    x2 = _rand((K, M), 64, 1.0, 0.2)
    za = ops.conv_bn_act(x, w4, gamma, beta, rm.clone(), rv.clone(), True, act=ops.ACT_RELU)
    zb = ops.conv_bn_act(x2, w4, gamma, beta, rm.clone(), rv.clone(), True, act=ops.ACT_RELU)
    with ops.defer_wgrad_reduce():
        ((za.float() + zb.float()) * up).sum().backward()
        assert len(ops._WGRAD_PENDING) == 0
    w5 = w0.clone().requires_grad_(True)
    zb5 = ops.conv_bn_act(x2, w5, gamma, beta, rm.clone(), rv.clone(), True, act=ops.ACT_RELU)
    (zb5.float() * up).sum().backward()
    assert torch.allclose(w4.grad, once + w5.grad, rtol=1e-6, atol=1e-6 * float(once.abs().max()))
    assert not ops._WGRAD_SEEN_IDS


# weights used more than once per block: (R, K, groups, M, views) -- plain, grouped, ragged column range (from SHAPES)
_SHARED_SHAPES = [(128, 64, 1, 8192, 1), (128, 128, 4, 4096, 2), (64, 64, 1, 128 * 2 * 37, 2)]


class _FlushInBackward(torch.autograd.Function):
    """Identity whose backward flushes the queued weight-gradient reductions: a reader in the middle of backward, as
    dist.GradSync packing a complete bucket."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        from grafp_amd import ops
        ops.flush_wgrad_reduce()
        return g


def _shared_case(R, K, groups, M, views, order, seed):
    """Leaf weights (one per letter of `order`), one bf16 operand per use, one upstream gradient per use and pass."""
    gen = torch.Generator().manual_seed(seed)
    names = sorted(set(order) - {"|"})
    w0 = {c: (0.2 * torch.randn(R, K // groups, generator=gen)).to(DEV) for c in names}
    uses = [c for c in order if c != "|"]
    xs = [_rand((K, M), seed + 10 + i, 1.0, 0.2) for i in range(len(uses))]
    ups = [[_rand((R, M), seed + 100 * (p + 1) + i).float() for i in range(len(uses))] for p in range(2)]
    return w0, xs, ups


def _shared_loss(ws, order, xs, ups, groups, views, only=None):
    """sum over the uses of <up, conv_bn_act(x, W)>; '|' puts a _FlushInBackward on the partial sum so far (its backward
    runs after that of every later use and before that of every earlier one).  only: that use alone."""
    from grafp_amd import ops
    R = next(iter(ws.values())).shape[0]
    gamma, beta = torch.ones(R, device=DEV), torch.zeros(R, device=DEV)
    loss, i = None, 0
    for c in order:
        if c == "|":
            loss = loss if loss is None else _FlushInBackward.apply(loss)
            continue
        if only is None or only == i:
            rm, rv = torch.zeros(R, device=DEV), torch.ones(R, device=DEV)
            z = ops.conv_bn_act(xs[i], ws[c], gamma, beta, rm, rv, True, act=ops.ACT_RELU, conv_groups=groups,
                                views=views)
            t = (z.float() * ups[i]).sum()
            loss = t if loss is None else loss + t
        i += 1
    return loss


def _shared_grads(w0, order, xs, ups, groups, views, defer, passes=1, flat=False):
    """.grad of every weight after `passes` backward passes, inside one defer_wgrad_reduce() block or without one;
    flat: under dist.GradSync(force_flat=True) (no process group: nothing is all-reduced), so the first gradient of each
    weight may be produced in its slice of the flat buffer.  -> ({name: grad}, {name: flat slice} or None)"""
    import contextlib
    from grafp_amd import dist as gdist, ops
    ws = {c: w.clone().requires_grad_(True) for c, w in w0.items()}
    sync = gdist.GradSync(list(ws.values()), force_flat=True) if flat else None
    try:
        if sync is not None:
            assert not sync._reduce and ops._GRAD_TARGET_OF is not None
            sync.zero()
        with ops.defer_wgrad_reduce() if defer else contextlib.nullcontext():
            for p in range(passes):
                _shared_loss(ws, order, xs, ups[p], groups, views).backward()
        assert ops._WGRAD_PENDING is None and not ops._WGRAD_SEEN_IDS
        slices = None
        if sync is not None:
            sync.finish()
            slices = {c: sync._view[id(w)].clone() for c, w in ws.items()}
            assert all(w.grad.data_ptr() == sync._view[id(w)].data_ptr() for w in ws.values())
    finally:
        if sync is not None:
            sync.close()
    assert ops._GRAD_TARGET_OF is None
    return {c: w.grad.clone() for c, w in ws.items()}, slices


def _count_deferred(monkeypatch):
    """Counts the weight gradients whose reduction was queued: every flush records the queue length it reduces."""
    from grafp_amd import ops
    real, counted = ops.flush_wgrad_reduce, []

    def counting_flush():
        counted.append(len(ops._WGRAD_PENDING or []))
        real()
    monkeypatch.setattr(ops, "flush_wgrad_reduce", counting_flush)
    return counted


def _single_use_f64(w0, order, xs, ups_pass, groups, views):
    """Per weight: the float64 sum of its gradients, each use differentiated ALONE (no deferral block)."""
    want = {c: torch.zeros(w.shape, dtype=torch.float64, device=DEV) for c, w in w0.items()}
    uses = [c for c in order if c != "|"]
    for i, c in enumerate(uses):
        ws = {k: w.clone().requires_grad_(True) for k, w in w0.items()}
        _shared_loss(ws, order, xs, ups_pass, groups, views, only=i).backward()
        want[c] += ws[c].grad.double()
    return want


def _assert_close_f64(got, want, what):
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    assert scale > 0 and err <= 1e-6 * scale, (what, err, scale)


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("order", ["ABAB", "ABBA", "AAA", "ABCCBA"])
@pytest.mark.parametrize("R,K,groups,M,views", _SHARED_SHAPES)
def test_deferred_weight_gradients_of_shared_weights(R, K, groups, M, views, order, flat, monkeypatch):
    """Weights used more than once in one backward pass inside ops.defer_wgrad_reduce(): only the FIRST gradient of each
    weight may stay unreduced; a later one flushes and reduces at once, also after a flush in between (A B A B: the flush
    of A's second use must not forget B, or B's second gradient is queued too and autograd adds unreduced memory --
    under the flat buffer the same slice twice).  Every .grad equals the run without a deferral block bit for bit and
    the float64 sum of the per-use gradients; each weight's first gradient is still deferred; flat: every slice of the
    flat buffer holds the gradient after finish()."""
    w0, xs, ups = _shared_case(R, K, groups, M, views, order, 70)
    want, _ = _shared_grads(w0, order, xs, ups, groups, views, defer=False)
    want64 = _single_use_f64(w0, order, xs, ups[0], groups, views)
    counted = _count_deferred(monkeypatch)
    got, slices = _shared_grads(w0, order, xs, ups, groups, views, defer=True, flat=flat)
    for c in w0:
        assert torch.isfinite(got[c]).all(), c
        assert torch.equal(got[c], want[c]), c
        _assert_close_f64(got[c], want64[c], c)
        if flat:
            assert torch.equal(slices[c], want[c]), c
    assert sum(counted) == len(w0), counted              # one deferred reduction per weight: its first gradient


@pytest.mark.parametrize("order", ["A", "ABAB"])
@pytest.mark.parametrize("R,K,groups,M,views", _SHARED_SHAPES)
def test_deferred_weight_gradients_of_two_backward_passes_in_one_block(R, K, groups, M, views, order, monkeypatch):
    """Gradient accumulation inside ONE defer_wgrad_reduce() block: the second pass finds .grad set by the first, whose
    reduction is still queued -- it must flush before AccumulateGrad adds to it (otherwise the sum is made of unreduced
    memory and the flush at the end of the block overwrites it with the first pass's gradient: the second is lost).
    .grad equals the two passes without the block bit for bit and the float64 sum of the two single-pass gradients."""
    w0, xs, ups = _shared_case(R, K, groups, M, views, order, 80)
    want, _ = _shared_grads(w0, order, xs, ups, groups, views, defer=False, passes=2)
    one = [_shared_grads(w0, order, xs, [ups[p]], groups, views, defer=False)[0] for p in range(2)]
    counted = _count_deferred(monkeypatch)
    got, _ = _shared_grads(w0, order, xs, ups, groups, views, defer=True, passes=2)
    for c in w0:
        assert torch.isfinite(got[c]).all(), c
        assert torch.equal(got[c], want[c]), c
        _assert_close_f64(got[c], one[0][c].double() + one[1][c].double(), c)
    assert sum(counted) == len(w0), counted              # the first pass's first gradients; nothing of the second pass


@pytest.mark.parametrize("order", ["A|A", "AB|BA"])
@pytest.mark.parametrize("R,K,groups,M,views", _SHARED_SHAPES)
def test_deferred_weight_gradients_with_a_flush_between_two_uses(R, K, groups, M, views, order, monkeypatch):
    """A flush in the middle of backward (what GradSync does when a bucket is complete) between two uses of the same
    weight: the second use must still be reduced at once -- the flush does not make the weight new again."""
    w0, xs, ups = _shared_case(R, K, groups, M, views, order, 90)
    want, _ = _shared_grads(w0, order, xs, ups, groups, views, defer=False)
    want64 = _single_use_f64(w0, order, xs, ups[0], groups, views)
    counted = _count_deferred(monkeypatch)
    got, _ = _shared_grads(w0, order, xs, ups, groups, views, defer=True)
    for c in w0:
        assert torch.isfinite(got[c]).all(), c
        assert torch.equal(got[c], want[c]), c
        _assert_close_f64(got[c], want64[c], c)
    assert sum(counted) == len(w0) and len(counted) >= 2, counted


@pytest.mark.parametrize("R,K,M", [(64, 64, 8192), (256, 64, 16384), (64, 256, 131072), (1024, 256, 4096), (512, 2048, 1024),
                                   (128, 96, 128 * 37), (2048, 512, 2560)])
def test_split_bf16_product_of_the_f32_mode(R, K, M):
    """ops.split_gemm_f32 (the f32 mode's forward / data-gradient products on the bf16 matrix cores): operands split into
    hi + lo bf16 planes (exact to 2^-17), y = Wh Xh + Wh Xl + Wl Xh in f32 accumulators.  Against a float64 product of the
    f32 operands: <= 3e-5 of the result's scale (the library's f32 GEMM: ~1e-6; bf16 operands alone: 4e-3) on every tile
    configuration the plan picks for these shapes."""
    from grafp_amd import ops
    assert not ops.switches.f32_split_gemm            # opt-in: 2^-16 per product is outside the f32 mode's 1e-4 bars
    g = torch.Generator().manual_seed(R + K)
    w = (0.2 * torch.randn(R, K, generator=g)).to(DEV)
    x = (torch.randn(K, M, generator=g) + 0.3).to(DEV)
    hi, lo = ops.split_planes(x)
    assert float((x - hi.float() - lo.float()).abs().max()) <= 2.0 ** -16 * float(x.abs().max())
    y = ops.split_gemm_f32(w, x)
    ref = (w.double() @ x.double())
    scale = float(ref.abs().max())
    assert float((y.double() - ref).abs().max()) <= 3e-5 * scale, float((y.double() - ref).abs().max()) / scale
    assert float((torch.mm(w.to(torch.bfloat16).float(), x.to(torch.bfloat16).float()).double() - ref).abs().max()) > 1e-3 * scale
    assert torch.equal(y, ops.split_gemm_f32(w, x))


# ---- every form of gemm_run on every tile configuration, and every weight-gradient tile, BIT FOR BIT ----------------------
# Operands on the grid of tests/_gemm_ref.py: every partial sum, in any order, is exact in f32, so the accumulator holds the
# exact value whatever the tile, ring depth, split-K cut or reduction order, and the output is that value rounded once.  The
# float64 reference rounded the same way must equal the kernel's output on every element (torch.equal, no allowance); outputs
# are allocated by the ops on the session's NaN-poisoned allocator, so an element nobody wrote fails too.
import _gemm_ref as gr  # noqa: E402

_EXACT_DEV = {"shape": None, "moved": {}, "refs": {}}


def _exact_operands(case):
    """The operands of a case on the device.  Consecutive cases of a shape share w / x / g (the makers return the same CPU
    tensor for the same name) and the references made from them; a new shape drops what the last one held."""
    st = _EXACT_DEV
    key = (case in gr.WGRAD_CASES, case.shape)
    if st["shape"] != key:
        st.update(shape=key, moved={}, refs={})
    out = {}
    for k, v in gr.case_operands(case).items():
        if torch.is_tensor(v):
            if id(v) not in st["moved"]:
                st["moved"][id(v)] = (v, v.to(DEV))
            out[k] = st["moved"][id(v)][1]
        else:
            out[k] = (v[0].to(DEV), v[1], v[2])
    return out


def _exact_product(case, o):
    """The float64 product of a case on the device, rounded as the kernel's output is, made once per (shape, prologue):
    the plain, statistics, epilogue and concatenated-operand forms share one (W [x1; x2] = W x)."""
    R, K, groups, M, views = case.shape
    key = ("pro", case.arg) if case.form in ("pro", "pro_stats") else ("f32", case.arg) if case.form == "f32" else "plain"
    refs = _EXACT_DEV["refs"]
    if key not in refs:
        refs[key] = gr.product(o["w"], o["x"], groups, views, o.get("pro"), None, DEV,
                               torch.float32 if case.form == "f32" else torch.bfloat16)
    return refs[key]


def _check_exact_partials(y, part, info, shape):
    """The statistics partials of a STATS launch against float64 on y: the layout walk and the bars of
    test_gemm_partials_against_float64 (a division is involved: the statistics are not exact on this grid either)."""
    R, K, groups, M, views = shape
    Mg, cols, P = M // views, info[2] * info[6], info[3]
    assert part.shape == (R, views, P, 3) and P == -(-Mg // cols)
    yv = y.float().double().reshape(R, views, Mg)
    full = Mg // cols
    segs = [yv[:, :, :full * cols].reshape(R, views, full, cols)] + ([yv[:, :, full * cols:, None].transpose(2, 3)] if P > full else [])
    mean = torch.cat([s.mean(dim=3) for s in segs], dim=2)
    m2 = torch.cat([((s - s.mean(dim=3, keepdim=True)) ** 2).sum(dim=3) for s in segs], dim=2)
    got = part.double()
    assert bool((part[..., 0] == 0).all())
    np.testing.assert_allclose(got[..., 2].cpu().numpy(), mean.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[..., 1].cpu().numpy(), m2.cpu().numpy(), rtol=4e-5)


def _where_differs(got, want):
    """For the message of a failed comparison: how many elements differ, in which rows and columns, and the first one."""
    bad = (got != want) | torch.isnan(got.float())
    rows, cols = bad.any(dim=1).nonzero().flatten(), bad.any(dim=0).nonzero().flatten()
    r, c = int(rows[0]), int(bad[int(rows[0])].nonzero()[0])
    return (f"{int(bad.sum())} of {bad.numel()} differ: rows {int(rows[0])}..{int(rows[-1])} ({rows.numel()}), columns "
            f"{int(cols[0])}..{int(cols[-1])} ({cols.numel()}); first [{r}, {c}]: got {float(got[r, c])}, want {float(want[r, c])}")


def _exact_launch(case, o):
    """-> (output, statistics partials or None) of the case's entry point."""
    from grafp_amd import ops
    R, K, groups, M, views = case.shape
    if case.form == "f32":
        return ops.split_gemm_f32(o["w"], o["x"]), None
    if case.form == "cat":
        return ops.conv1x1_gemm_cat(o["w"], o["x"][:case.arg], o["x"][case.arg:]), None
    if case.form == "epi":
        tab, act, slope = o["epi"]
        return ops.conv1x1_gemm_affine(o["w"], o["x"], tab, groups, views, act=act, slope=slope), None
    tab, act, slope = o.get("pro", (None, 0, 0.0))
    got = ops.conv1x1_gemm(o["w"], o["x"], groups, views, pro_tab=tab, pro_act=act, pro_slope=slope,
                           stats=case.form in ("stats", "pro_stats"))
    return got if isinstance(got, tuple) else (got, None)


@pytest.mark.parametrize("name", [c.name for c in gr.GEMM_CASES])
def test_gemm_equals_float64_bit_for_bit_on_exact_operands(name):
    """One cell of the form x tile matrix (tests/_gemm_ref.py: CASES): the plan rule sends the shape to the expected tile
    configuration (an XL plan runs the forms the four-wave tile lacks on the L tile), the operands pass check_grid, and
    the output of two launches equals the float64 reference on every element -- the product rounded once to bf16; with an
    affine epilogue the rounded product, transformed, rounded once more; for the f32 output the product itself, with
    ops.split_planes returning the exact hi + lo of both operands.  A statistics form leaves the bits of y alone; its
    partials are held against float64 on y with the bars of test_gemm_partials_against_float64."""
    from grafp_amd import ops
    case = gr.CASE_BY_NAME[name]
    R, K, groups, M, views = case.shape
    info = _plan_info(R, 3 * K if case.form == "f32" else K, groups, M, views)
    assert info[0] == case.plan, (name, info)
    o = _exact_operands(case)
    gr.check_grid(case, o)
    want = _exact_product(case, o)
    if case.form == "epi":
        want = gr.affine(want, o["epi"], views)
    if case.form == "f32":
        for t in (o["w"], o["x"]):
            hi, lo = ops.split_planes(t)
            assert torch.equal(hi.float() + lo.float(), t)
    first, part1 = _exact_launch(case, o)
    assert first.dtype == want.dtype and first.shape == want.shape
    assert torch.equal(first, want), (name, _where_differs(first, want))
    if part1 is not None:
        _check_exact_partials(first, part1, info, case.shape)
    again, part2 = _exact_launch(case, o)
    assert torch.equal(again, first) and (part1 is None or torch.equal(part1, part2))


def test_normalise_on_load_on_the_128_row_tile_refuses_more_than_1024_operand_rows():
    """The one cell of the matrix that the library refuses by shape (tests/_gemm_ref.py: REFUSED): a prologue table of an
    N128-planned product with more than 1024 operand rows per group does not fit beside the ring."""
    from grafp_amd import ops
    R, K, M = 128, 1056, 131072
    assert _plan_cfg(R, K, 1, M, 1) == gr.CFG_N128 and K > gr.N128_PRO_MAX_KG
    w = torch.ones((R, K), dtype=torch.bfloat16, device=DEV)
    x = torch.ones((K, M), dtype=torch.bfloat16, device=DEV)
    tab = gr.affine_table("ge:refused.pro", K, 1).to(DEV)
    with pytest.raises(RuntimeError, match="at most 1024 operand rows"):
        ops.conv1x1_gemm(w, x, 1, 1, pro_tab=tab, pro_act=ops.ACT_RELU)


@pytest.mark.parametrize("name", [c.name for c in gr.WGRAD_CASES])
def test_wgrad_equals_float64_bit_for_bit_on_exact_operands(name):
    """The weight gradient on exact operands (f32 output: the float64 product itself): every LDS-DMA tile forced, plain
    and with the normalise-on-load operand (T128 / S128 on shapes whose views are no whole 128-column chunks run T / S),
    the register-staged kernel on both tile widths, and the f32 route (split-bf16 planes, through
    ops.conv1x1_rows(...).backward) with the low plane on either operand.  Two launches, identical bits."""
    import ctypes
    from grafp_amd import ops
    from grafp_amd._lib import lib
    case = gr.CASE_BY_NAME[name]
    cout, cin, groups, M, views = case.shape
    o = _exact_operands(case)
    gr.check_grid(case, o)
    info = (ctypes.c_int * 8)()
    assert lib.grafp_conv1x1_wgrad_plan(cout, cin, groups, M, views, info) == 0
    if case.entry == "conv1x1_wgrad":
        # a forced tile is honoured on an LDS-DMA shape only; plan code -1 is the register-staged kernel
        assert (info[0] == -1) == (case.plan == -1), (name, list(info))
        if case.plan == -1:
            assert info[1] == dict(gr.WG_REG_SHAPES)[case.shape]
        tab, act, slope = o.get("pro", (None, ops.ACT_NONE, 0.0))

        def run():
            return ops.conv1x1_wgrad(o["g"], o["x"], cout, cin, groups, M, views, tab, act, slope, tile=case.plan)
    else:
        assert not ops.switches.wgrad_f32_library

        def run():
            w = torch.zeros((cout, cin // groups), device=DEV, requires_grad=True)
            ops.conv1x1_rows(o["x"], w, groups).backward(o["g"])
            return w.grad
    refs = _EXACT_DEV["refs"]
    key = (case.form, case.arg)                 # plain: the tiles of a shape share one reference
    if key not in refs:
        refs[key] = gr.wgrad(o["g"], o["x"], groups, views, o.get("pro"), DEV)
    want = refs[key]
    first = run()
    assert first.dtype == torch.float32 and first.shape == want.shape
    assert torch.equal(first, want), (name, _where_differs(first, want))
    assert torch.equal(run(), first)
