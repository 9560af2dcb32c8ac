"""CPU tests of what the bit-for-bit GPU tests of the 1x1 GEMM and the weight gradient stand on (tests/_gemm_ref.py): the
grid condition holds for every case, the plan queries (pure host functions) send every case to the tile its row of the
table names and the table covers the form x tile matrix, f32 sums of the operands are exact in any order, one grid step
on any operand element moves the reference, and the deep products do exercise the bf16 rounding rule."""
import ctypes

import pytest
import torch

import _gemm_ref as gr

SMALL_M = 1280
SMALL = [c for c in gr.CASES if c.shape[3] <= SMALL_M]


def _gemm_plan(R, K, groups, M, views):
    from grafp_amd._lib import lib
    info = (ctypes.c_int * 8)()
    assert lib.grafp_conv1x1_gemm_plan(R, K, groups, M, views, info) == 0
    return list(info)


def _wgrad_plan(cout, cin, groups, M, views):
    from grafp_amd._lib import lib
    info = (ctypes.c_int * 8)()
    assert lib.grafp_conv1x1_wgrad_plan(cout, cin, groups, M, views, info) == 0
    return list(info)


def _shapes(cases):
    return list(dict.fromkeys((c in gr.WGRAD_CASES, c.shape) for c in cases))


@pytest.mark.parametrize("wg,shape", _shapes(gr.CASES))
def test_check_grid_holds_for_every_case(wg, shape):
    """check_grid on the operands as the GPU test hands them over (generated in bf16 / f32, the 134 MB ones included), for
    every case of the shape.  Its bound on sum |a| |b| is analytic: contraction length x the largest |a| x the largest
    |b| of the operands at hand (|hi| + |lo| for a split route, the largest transformed grid value under a prologue
    table), which no drawn sum can exceed."""
    cases = [c for c in (gr.WGRAD_CASES if wg else gr.GEMM_CASES) if c.shape == shape]
    assert cases
    for case in cases:
        bound = gr.check_grid(case, gr.case_operands(case))
        assert 0 < bound < gr.SUM_CAP


def test_check_grid_refuses_what_breaks_the_argument():
    case = gr.CASE_BY_NAME["S-64x64g1x256v2-plain"]
    good = gr.case_operands(case)
    for key, pos, value in (("w", (3, 5), 0.0), ("w", (3, 5), 5.0), ("x", (7, 9), 0.5), ("x", (7, 9), 9.0)):
        bad = dict(good)
        bad[key] = good[key].clone()
        bad[key][pos] = value
        with pytest.raises(AssertionError):
            gr.check_grid(case, bad)
    deep = gr.Case("too-deep", "conv1x1_gemm", "plain", (32, 1 << 17, 1, 128, 1), 0, None)
    with pytest.raises(AssertionError):
        gr.check_grid(deep, {"w": torch.full((32, 1 << 17), 4.0).bfloat16(), "x": torch.full((1 << 17, 128), 8.0).bfloat16()})
    pro = gr.CASE_BY_NAME["S-64x64g1x256v2-pro2"]
    bad = dict(gr.case_operands(pro))
    tab = bad["pro"][0].clone()
    tab[5, 1, 0] = 0.75                                     # a scale off the grid: 11 significant bits at x = 7
    bad["pro"] = (tab, bad["pro"][1], bad["pro"][2])
    with pytest.raises(AssertionError):
        gr.check_grid(pro, bad)


def test_tables_differ_by_row_and_by_view():
    for rows, views in ((64, 2), (512, 2), (160, 3)):
        tab = gr.affine_table(f"t:{rows}.{views}", rows, views)
        assert tab.shape == (rows, views, 2) and tab.dtype == torch.float32
        for v in range(1, views):
            assert bool((tab[:, v, 0] != tab[:, v - 1, 0]).all()) and bool((tab[:, v, 1] != tab[:, v - 1, 1]).all())
        assert len({tuple(r.flatten().tolist()) for r in tab}) > rows // 2
        assert {float(s) for s in tab[..., 0].flatten()} == set(gr.SCALES)
        assert {float(s) for s in tab[..., 1].flatten()} == {float(s) for s in range(-gr.SHIFT_MAX, gr.SHIFT_MAX + 1)}


def test_plan_queries_send_every_case_to_its_tile():
    for case in gr.GEMM_CASES:
        R, K, groups, M, views = case.shape
        info = _gemm_plan(R, 3 * K if case.form == "f32" else K, groups, M, views)
        assert info[0] == case.plan, (case.name, info)
    for case in gr.WGRAD_CASES:
        info = _wgrad_plan(*case.shape)
        if case.entry == "conv1x1_wgrad":
            # a forced tile is honoured on an LDS-DMA shape only; -1: the register-staged kernel and its tile width
            assert (info[0] == -1) == (case.plan == -1), (case.name, info)
            if case.plan == -1:
                assert info[1] == info[2] == dict(gr.WG_REG_SHAPES)[case.shape]


def test_cases_cover_the_form_by_tile_matrix():
    """Every (tile configuration, form) cell has a case, but for what the library refuses (gr.REFUSED): the concatenated
    operand and the f32 output exist ungrouped with one view only (their entry points have no such arguments), and a
    prologue on N128 needs Kg <= 1024 (tests/test_gpu_gemm.py asks for that refusal on the device).  Likewise the weight
    gradient: every tile id plain, every id that has the form with a prologue, both register tile widths, the f32 route with
    the low plane on either side."""
    cells = {(c.plan, c.form) for c in gr.GEMM_CASES}
    assert cells == {(cfg, form) for cfg in gr.CFG_NAMES for form in gr.FORMS}
    for c in gr.GEMM_CASES:
        R, K, groups, M, views = c.shape
        if c.form in ("cat", "f32"):
            assert groups == 1 and views == 1, c.name
        if c.form in ("pro", "pro_stats") and c.plan == gr.CFG_N128:
            assert K // groups <= gr.N128_PRO_MAX_KG, c.name
    assert {key[0] for key in gr.REFUSED} == {"cat", "f32", "pro", "wgrad pro"}
    # every shape of the table runs every form its entry point accepts
    for shape, cfg in gr.GEMM_SHAPES:
        forms = {c.form for c in gr.GEMM_CASES if c.shape == shape and c.form != "f32"}
        R, K, groups, M, views = shape
        want = {"plain", "stats", "pro", "pro_stats", "epi"} | ({"cat"} if groups == 1 and views == 1 and K >= 64 else set())
        assert forms == want, shape
        for form in ("pro", "pro_stats", "epi"):
            assert {c.arg for c in gr.GEMM_CASES if c.shape == shape and c.form == form} == {0, 1, 2}
    # the fallback of gemm_run (a form the four-wave tile lacks runs on the L tile with the XL plan): three shapes a form
    for form in ("pro", "pro_stats", "epi"):
        assert len({c.shape for c in gr.GEMM_CASES if c.plan == gr.CFG_XL and c.form == form}) == 3
    assert any(c.plan == gr.CFG_XL and c.form == "f32" for c in gr.GEMM_CASES)
    # ragged rows (rows per group no multiple of the tile's) under the concatenated operand, groups under a prologue on an
    # N tile
    assert any(c.form == "cat" and c.shape[0] % 128 for c in gr.GEMM_CASES if c.plan == gr.CFG_S)
    assert any(c.form == "cat" and c.shape[0] % 128 for c in gr.GEMM_CASES if c.plan == gr.CFG_N128)
    assert any(c.form == "pro" and c.shape[2] > 1 for c in gr.GEMM_CASES if c.plan == gr.CFG_N32)
    # cat: both ends and a cut that is not the middle
    for K in sorted({c.shape[1] for c in gr.GEMM_CASES if c.form == "cat"}):
        cuts = gr.cat_splits(K)
        assert all(k % 32 == 0 and 0 < k < K for k in cuts) and 32 in cuts and K - 32 in cuts
        assert K < 192 or any(k not in (32, K - 32, K // 2) for k in cuts)
        assert {c.arg for c in gr.GEMM_CASES if c.form == "cat" and c.shape[1] == K} == set(cuts)
    wg = [c for c in gr.WGRAD_CASES if c.entry == "conv1x1_wgrad"]
    for shape in gr.WG_SHAPES:
        assert {c.plan for c in wg if c.shape == shape and c.form == "plain"} == set(gr.WG_TILES)
        assert {c.plan for c in wg if c.shape == shape and c.form == "pro"} == set(gr.WG_PRO_TILES)
    assert {c.arg for c in wg if c.form == "pro"} == {gr.ACT_RELU, gr.ACT_LEAKY}
    for tile in gr.WG_PRO_TILES:
        assert {c.arg for c in wg if c.form == "pro" and c.plan == tile} == {gr.ACT_RELU, gr.ACT_LEAKY}
    # T128 / S128 with views that are no whole 128-column chunks (the documented fall-back to T / S), and with whole ones
    for tile in gr.WG_CHUNK128_TILES:
        rest = {(c.shape[3] // c.shape[4]) % 128 != 0 for c in wg if c.plan == tile}
        assert rest == {True, False}
    assert {tw for _s, tw in gr.WG_REG_SHAPES} == {64, 128}
    assert {c.shape[:4] for c in gr.WGRAD_CASES if c.form == "f32"} == set(gr.WG_F32_SHAPES)
    for shape in gr.WG_F32_SHAPES:
        assert {c.arg for c in gr.WGRAD_CASES if c.form == "f32" and c.shape[:4] == shape} == {"wide_g", "wide_x"}


# ---- the exactness claim itself, on the CPU ------------------------------------------------------------------------------
def _f32_factors(case, o):
    """Per row group the f32 matrices (A, B) whose product over the contraction is the case's result before the output
    rounding: A (rows, L), B (L, columns); a split route's three plane products side by side (L = 3 x the contraction)."""
    R, K, groups, M, views = case.shape
    wgrad = "g" in o
    a = o["g" if wgrad else "w"].float()
    x = gr.transformed(o["x"], o["pro"], views).float() if "pro" in o else o["x"].float()
    out = []
    for i in range(groups):
        ai = a[i * (R // groups):(i + 1) * (R // groups)]
        xi = x[i * (K // groups):(i + 1) * (K // groups)]
        if case.form == "f32":
            (ah, al), (xh, xl) = gr.planes(ai), gr.planes(xi)
            if wgrad:
                out.append((torch.cat((al, ah, ah), dim=1), torch.cat((xh, xl, xh), dim=1).t()))
            else:
                out.append((torch.cat((ah, ah, al), dim=1), torch.cat((xh, xl, xh), dim=0)))
        else:
            out.append((ai, xi.t() if wgrad else xi))
    return out


def _finish(case, o, y):
    R, K, groups, M, views = case.shape
    if "g" in o or case.form == "f32":
        return y
    y = y.to(torch.bfloat16)
    return gr.affine(y, o["epi"], views) if "epi" in o else y


# plain and statistics forms, and the cuts of a concatenated operand, are one product: the plain case stands for them; the
# weight-gradient tiles share their operands: the first plain and the first prologue case of a shape stand for the rest
_DISTINCT = [c for c in SMALL if c.form not in ("stats", "pro_stats", "cat") and
             (c.entry != "conv1x1_wgrad" or c.plan in (0, -1))]


@pytest.mark.parametrize("name", [c.name for c in _DISTINCT])
def test_f32_sums_equal_float64_in_any_order(name):
    """f32 torch products of the operands equal the float64 reference exactly: in natural order, under a random permutation
    of the contraction, and summed in 32- and 128-wide chunks (every chunk an f32 product, the chunks added in f32, forwards
    and backwards)."""
    case = gr.CASE_BY_NAME[name]
    o = gr.case_operands(case)
    want = gr.case_reference(case, o)
    factors = _f32_factors(case, o)
    L = factors[0][0].shape[1]
    perm = torch.randperm(L, generator=torch.Generator().manual_seed(L))

    def chunked(A, B, width, backwards):
        cuts = list(range(0, L, width))
        acc = torch.zeros((A.shape[0], B.shape[1]), dtype=torch.float32)
        for c0 in (reversed(cuts) if backwards else cuts):
            acc = acc + A[:, c0:c0 + width] @ B[c0:c0 + width]
        return acc
    orders = {
        "natural": lambda A, B: A @ B,
        "permuted": lambda A, B: A[:, perm] @ B[perm],
        "chunks of 32": lambda A, B: chunked(A, B, 32, False),
        "chunks of 128, backwards": lambda A, B: chunked(A, B, 128, True),
    }
    for what, f in orders.items():
        y = torch.cat([f(A, B) for A, B in factors], dim=0)
        assert y.dtype == torch.float32
        got = _finish(case, o, y)
        assert got.dtype == want.dtype and torch.equal(got, want), (name, what)


def _positions(rows, cols, seed, n=12):
    g = torch.Generator().manual_seed(seed)
    corners = [(0, 0), (rows - 1, cols - 1), (rows - 1, 0), (0, cols - 1)]
    return corners + list(zip(torch.randint(0, rows, (n,), generator=g).tolist(), torch.randint(0, cols, (n,), generator=g).tolist()))


@pytest.mark.parametrize("name", [c.name for c in _DISTINCT if c.form in ("plain", "f32")])
def test_one_grid_step_on_any_element_moves_the_reference(name):
    """Changing a single operand element by one grid step changes the reference: 16 positions per operand, the corners
    among them -- the last column (of a ragged last slice), the last row (of a ragged last row tile) and the last k.
    Only the outputs an element reaches are recomputed: a column of y for x[k, m], a row for w[r, k]."""
    case = gr.CASE_BY_NAME[name]
    R, K, groups, M, views = case.shape
    o = gr.case_operands(case)
    wgrad = "g" in o
    a, x = o["g" if wgrad else "w"], o["x"]
    rg, kg = R // groups, K // groups
    out_dtype = torch.float32 if (wgrad or case.form == "f32") else torch.bfloat16

    def reach(a_, x_, grp):
        """The reference of row group grp from the operand slices a_ (rows of the group) and x_ (rows of the group)."""
        if wgrad:
            return gr.wgrad(a_, x_)
        return gr.product(a_, x_, out_dtype=out_dtype)
    for (r, c) in _positions(*a.shape, seed=R + K):
        grp = r // rg
        xs = x[grp * kg:(grp + 1) * kg]
        row = a[r:r + 1].clone()
        before = reach(row, xs, grp)
        row[0, c] += 1.0 if float(row[0, c]) != -1.0 else -1.0          # stays non-zero
        assert not torch.equal(reach(row, xs, grp), before), (name, "left operand", r, c)
    for (k, m) in _positions(*x.shape, seed=K + M):
        grp = k // kg
        as_ = a[grp * rg:(grp + 1) * rg]
        if wgrad:
            rows = x[k:k + 1].clone()                                    # one row of x reaches one column of dW
            before = reach(as_, rows, grp)
            rows[0, m] += 1.0
            after = reach(as_, rows, grp)
        else:
            col = x[grp * kg:(grp + 1) * kg, m:m + 1].clone()            # one column of x reaches one column of y
            before = reach(as_, col, grp)
            col[k - grp * kg, 0] += 1.0
            after = reach(as_, col, grp)
        assert not torch.equal(after, before), (name, "x", k, m)


@pytest.mark.parametrize("shape,cfg", [(s, c) for s, c in gr.GEMM_SHAPES if s[1] // s[2] >= 256])
def test_deep_products_exercise_the_rounding_rule(shape, cfg):
    """K >= 256: at least 1 % of the bf16 outputs are not representable before the rounding and some of those are exact
    ties, so a truncating store or a wrong tie rule fails the bit-for-bit comparison.  (The first 2048 columns of the long
    shapes: the columns are identically distributed.)"""
    R, K, groups, M, views = shape
    case = next(c for c in gr.GEMM_CASES if c.shape == shape and c.form == "plain")
    o = gr.case_operands(case)
    w, x = o["w"].double(), o["x"][:, :2048].double()
    y = torch.cat([w[i * (R // groups):(i + 1) * (R // groups)] @ x[i * (K // groups):(i + 1) * (K // groups)]
                   for i in range(groups)], dim=0)
    lo = y.float().to(torch.bfloat16).double()
    inexact = y != lo
    # the two bf16 neighbours of an inexact y: a tie is at the same distance from both
    step = 2.0 ** (torch.floor(torch.log2(y.abs().clamp(min=1.0))) - 7)
    down = torch.floor(y / step) * step
    tie = inexact & ((y - down) == (down + step - y))
    assert float(inexact.double().mean()) >= 0.01, float(inexact.double().mean())
    assert int(tie.sum()) > 0
    # ... and both tie directions occur: to the even neighbour below and to the even neighbour above
    assert bool((lo[tie] < y[tie]).any()) and bool((lo[tie] > y[tie]).any())


@pytest.mark.parametrize("name", [c.name for c in gr.CASES if c.form == "f32" and c.shape[3] <= 65536])
def test_split_grid_planes(name):
    """hi + lo reconstructs the wide operand exactly with lo != 0 somewhere (often: most of its values are above 256 and
    half of them odd); the narrow operand's lo is zero everywhere; the dropped lo * lo term is therefore zero."""
    case = gr.CASE_BY_NAME[name]
    o = gr.case_operands(case)
    a, x = o["g" if "g" in o else "w"], o["x"]
    wide, narrow = (x, a) if case.arg == "wide_x" else (a, x)
    hi, lo = gr.planes(wide)
    assert torch.equal(hi + lo, wide) and float((lo != 0).float().mean()) > 0.2
    assert float(wide.abs().max()) > 256 and float((wide % 2 != 0).float().mean()) > 0.3
    nh, nl = gr.planes(narrow)
    assert torch.equal(nh, narrow) and not bool(nl.any())
