"""GPU tests of normalise-on-load (the PRO forms of gemm.hip and wgrad.hip, one kernel per activation code): every tile
configuration that has the form, on the smallest shapes that reach its edges, bit for bit against the separate pass
(bn_affine) followed by the plain product / plain weight gradient of the same library.  `pytest -m gpu`."""
import pytest
import torch

from test_gpu_gemm import DEV, _plan_info

pytestmark = pytest.mark.gpu

SLOPE = 0.2
# tile configuration numbers of the plan query (gemm.hip GM_CFG_*)
S, L, N32, N64, N128, XL = 0, 1, 2, 3, 4, 5

# ((R, K, groups, M, views), the plan's tile, activation code).  Per tile: two views whose column ranges are full ones and a
# short last one, and a shape whose K per group is ONE chunk of 32 (N128 starts at K = 128: none).  The rule sends only
# >= 2^16 (N32, N64) / 2^17 (N128) columns per view to the 512-column tiles.  An XL plan runs its PRO form on the L tile
# (the four-wave tile has none) on the XL plan's grid.  The three activation codes go round the list.
PRODUCTS = [((64, 64, 1, 9472, 2), S, 1), ((96, 32, 1, 1280, 1), S, 2),
            ((512, 64, 1, 4608, 2), L, 0), ((512, 32, 1, 2560, 1), L, 1),
            ((256, 512, 1, 2 * 256 * 257, 2), XL, 2),      # (>= 16 chunks per tile: ranges of two tiles only from 257 tiles per view)
            ((32, 64, 1, 2 * 512 * 131, 2), N32, 0), ((32, 32, 1, 512 * 131, 1), N32, 1),
            ((64, 64, 1, 2 * 512 * 131, 2), N64, 2), ((64, 32, 1, 512 * 131, 1), N64, 0),
            ((128, 512, 1, 2 * 512 * 257, 2), N128, 1), ((96, 160, 1, 512 * 1025, 1), N128, 2)]

# weight gradient: T, S, L, S32, M32, L32, T128, S128 (wgrad.hip WgTileId), forced through `tile` for the PRO launch and
# for the plain one, so that both cut the same slices.  (cout, cin, groups, M, views): two views with nine full slices
# and a short one; ragged rows on both sides with a short last slice; one chunk per slice of the tile's chunk length
# (two chunks for the 32-column tiles: a view is a multiple of 64 columns)
WG_TILES = {0: 64, 1: 64, 2: 64, 3: 32, 4: 32, 5: 32, 8: 128, 10: 128}
WG_SHAPES = [(64, 64, 1, 9472, 2), (96, 160, 1, 1280, 1), (128, 256, 1, None, 1)]


def _operands(rows, K, M, views, seed):
    """bf16 operands drawn on the device, and a (K, views, 2) table of (scale, shift)."""
    torch.manual_seed(seed)
    a = (torch.randn(rows, M, device=DEV)).to(torch.bfloat16)
    x = (torch.randn(K, M, device=DEV) * 2.0 + 1.0).to(torch.bfloat16)
    tab = torch.stack((torch.rand(K, views, device=DEV) + 0.5, torch.randn(K, views, device=DEV)), dim=-1).contiguous()
    return a, x, tab


def _assert_partials_match_float64(part, y, shape):
    """The statistics partials against float64 on the rounded y: the layout and the two bars of
    tests/test_gpu_gemm.py::test_gemm_partials_against_float64 (mean: rtol 1e-5 + atol 1e-5; M2: rtol 4e-5 -- literals there,
    so they cannot be imported and are repeated here, unchanged)."""
    import numpy as np
    R, K, groups, M, views = shape
    info = _plan_info(*shape)
    Mg, cols, P = M // views, info[2] * info[6], info[3]
    assert part.shape == (R, views, P, 3) and P == -(-Mg // cols)
    yv = y.float().double().reshape(R, views, Mg)
    full = Mg // cols
    segs = [yv[:, :, :full * cols].reshape(R, views, full, cols)] + ([yv[:, :, full * cols:, None].transpose(2, 3)] if P > full else [])
    mean = torch.cat([s.mean(dim=3) for s in segs], dim=2)
    m2 = torch.cat([((s - s.mean(dim=3, keepdim=True)) ** 2).sum(dim=3) for s in segs], dim=2)
    got = part.double()
    print(f"{shape}: {P} ranges of {cols} columns (last {Mg - (P - 1) * cols}); partials vs float64: mean "
          f"{float((got[..., 2] - mean).abs().max()):.3e} abs, M2 {float(((got[..., 1] - m2).abs() / m2).max()):.3e} rel")
    assert bool((part[..., 0] == 0).all())
    np.testing.assert_allclose(got[..., 2].cpu().numpy(), mean.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[..., 1].cpu().numpy(), m2.cpu().numpy(), rtol=4e-5)


@pytest.mark.parametrize("shape,cfg,act", PRODUCTS)
def test_product_with_normalise_on_load_is_the_separate_pass_bit_for_bit(shape, cfg, act):
    """y and (on the same tile) the statistics partials of the PRO + STATS product equal those of bn_affine + STATS product;
    y of the PRO product without statistics too; the partials agree with float64 on the rounded y.  Measured on the parent
    commit's library before the activation code became a template argument: every case bit-equal (deviation 0), so the bar
    is equality.  The XL plan's plain product runs on the four-wave tile and its PRO form on the eight-wave one: y is equal
    there too, the partials are merged over other wave columns and are held to the float64 bars only."""
    from grafp_amd import ops
    R, K, groups, M, views = shape
    info = _plan_info(*shape)
    assert info[0] == cfg, info[:4]
    assert info[3] > 1 and (M // views) % (info[2] * info[6]) != 0, "the last column range of a view is a short one"
    _, x, tab = _operands(1, K, M, views, 7 * R + K)
    w = (torch.randn(R, K // groups, device=DEV) * 0.2).to(torch.bfloat16)
    z = ops.bn_affine(x, tab, views, None, act, SLOPE)
    y0, p0 = ops.conv1x1_gemm(w, z, groups, views, stats=True)
    y1, p1 = ops.conv1x1_gemm(w, x, groups, views, pro_tab=tab, pro_act=act, pro_slope=SLOPE, stats=True)
    y2 = ops.conv1x1_gemm(w, x, groups, views, pro_tab=tab, pro_act=act, pro_slope=SLOPE)
    print(f"{shape} act {act}: y differs in {int((y1 != y0).sum())} (PRO + STATS), {int((y2 != y0).sum())} (PRO) of {y0.numel()}; "
          f"partials differ in {int((p1 != p0).sum())} of {p0.numel()}")
    assert torch.equal(y1, y0) and torch.equal(y2, y0)
    if cfg != XL:
        assert torch.equal(p1, p0)
    _assert_partials_match_float64(p1, y1, shape)


@pytest.mark.parametrize("tile", sorted(WG_TILES))
@pytest.mark.parametrize("case", range(len(WG_SHAPES)))
def test_weight_gradient_with_normalise_on_load_is_the_separate_pass_bit_for_bit(case, tile):
    """dW of the PRO launch equals dW of the plain launch on the materialised bn_affine output, same tile, same slices.
    Measured on the parent commit's library: every case bit-equal, so the bar is equality."""
    from grafp_amd import ops
    cout, cin, groups, M, views = WG_SHAPES[case]
    M = M or max(WG_TILES[tile], 64)
    act = (case + tile) % 3
    g, x, tab = _operands(cout, cin, M, views, 100 * case + tile)
    z = ops.bn_affine(x, tab, views, None, act, SLOPE)
    d0 = ops.conv1x1_wgrad(g, z, cout, cin, groups, M, views, tile=tile, may_defer=False)
    d1 = ops.conv1x1_wgrad(g, x, cout, cin, groups, M, views, tab, act, SLOPE, tile=tile, may_defer=False)
    print(f"{(cout, cin, groups, M, views)} tile {tile} act {act}: dW differs in {int((d1 != d0).sum())} of {d0.numel()}, "
          f"largest {float((d1 - d0).abs().max()):.3e}")
    assert d1.shape == (cout, cin // groups) and d1.dtype == torch.float32
    assert float(d0.abs().max()) > 0
    assert torch.equal(d1, d0)


def test_defer_norm_pays_follows_the_committed_table():
    """The rule of ops.defer_norm_pays on the consumers (gfc2: C x 2C, ffn2: C x 4C) of the encoder's twelve blocks
    (2, 2, 6, 2 per stage; C = 64 ... 512, N = 1024 ... 128 nodes), per stage what DESIGN.md 12.5 / profiles/
    pro_cost_bench_2048.txt say: stages 0-1 at every size, stages 2-3 never (stage 2 nets -11 / -18 us per layer at 2048
    clip-views, inside the spread of 11 / 27)."""
    from grafp_amd import ops
    assert ops.switches.defer_norm
    stages = ((64, 1024), (128, 512), (256, 256), (512, 128))
    blocks = [s for s, depth in enumerate((2, 2, 6, 2)) for _ in range(depth)]
    assert len(blocks) == 12
    for clips, want in ((2048, (True, True, False, False)), (512, (True, True, False, False))):
        for s in blocks:
            C, N = stages[s]
            for K in (2 * C, 4 * C):
                assert ops.defer_norm_pays(C, K, clips * N) is want[s], (clips, s, C, K)
