"""Exact operands, float64 references and the case table of the bit-for-bit tests of the 1x1 GEMM (gemm.hip, gemm_xl.h)
and the weight gradient (wgrad.hip) (TEST INFRASTRUCTURE): tests/test_gemm_exact_cpu.py pins them on the CPU, the end of
tests/test_gpu_gemm.py compares every form on every tile configuration with them by torch.equal.  Nothing here needs a GPU.

Exact, because the operands sit on a grid on which every partial sum, in ANY order, is exact in f32:
  * weights and gradients: non-zero integers in [-4, 4]; activations: integers in [-8, 8]; both are bf16 values;
  * a prologue table has scale in {+-0.5, +-1, +-2} and an integer shift in [-4, 4], the leaky slope is 0.25: act(x * scale
    + shift) is a multiple of 1/8 of at most 20, i.e. at most 8 significant bits -- an fma and a mul + add give the same
    value and the bf16 rounding of the transformed operand does nothing;
  * every product of two operand elements is then an integer number of grid units (1, or 1/8 with a prologue), and over the
    whole contraction sum |a| |b| stays below 2^22 units (check_grid): every partial sum of every summation tree -- tile, ring
    depth, split-K cut, final reduction -- is an integer below 2^22 and exact in f32's 24 bits with two bits to spare;
  * the f32 accumulator therefore holds the exact value; an f32 output is that value, a bf16 output that value rounded once,
    an affine epilogue (power-of-two scale, small integer shift) acts exactly on the rounded product and is rounded once more;
  * the split-bf16 routes of the f32 mode: one operand on the 8-bit grid above (its low plane is zero), the other a
    non-zero integer of 9-10 bits (its low plane is non-zero and exact); the dropped lo * lo term is exactly zero and
    Wh Xh + Wh Xl + Wl Xh is the full product.  Both assignments: each cross term is then the only carrier of the low
    bits in one of them.
The float64 references assert that their own result survives .float().double(), i.e. is exact in f32."""
import functools
import zlib
from collections import namedtuple

import torch

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
SLOPE = 0.25
W_MAX, X_MAX, SHIFT_MAX = 4, 8, 4
SCALES = (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
WIDE_MAX = 1023
SUM_CAP = 1 << 22                 # sum |a| |b| over a whole contraction, in grid units: two bits under f32's 24
PRO_UNIT = 8                      # a prologue-transformed operand is a multiple of 1 / PRO_UNIT

# tile configurations of gemm.hip (GM_CFG_*): info[0] of grafp_conv1x1_gemm_plan
CFG_S, CFG_L, CFG_N32, CFG_N64, CFG_N128, CFG_XL = 0, 1, 2, 3, 4, 5
CFG_NAMES = {CFG_S: "S", CFG_L: "L", CFG_N32: "N32", CFG_N64: "N64", CFG_N128: "N128", CFG_XL: "XL"}
# ((R, K, groups, M, views), configuration): per configuration the smallest shapes the plan rule sends there and what
# each adds
GEMM_SHAPES = [
    ((64, 64, 1, 256, 2), CFG_S),
    ((96, 32, 1, 384, 1), CFG_S),            # ragged rows
    ((288, 64, 1, 768, 1), CFG_S),           # three row tiles, the last one 32 rows; ranges of 4 + 2 tiles
    ((128, 128, 4, 1024, 2), CFG_S),         # grouped
    ((512, 64, 1, 512, 1), CFG_L),
    ((576, 64, 1, 768, 1), CFG_L),           # ragged last row tile
    ((320, 512, 1, 512, 1), CFG_L),          # Rg % 256 != 0 keeps it off XL
    ((256, 512, 1, 512, 2), CFG_XL),
    ((512, 512, 1, 768, 1), CFG_XL),         # P = 3
    ((256, 576, 1, 1280, 1), CFG_XL),        # K not a multiple of 128; odd tile count
    ((32, 32, 1, 65536, 1), CFG_N32),
    ((32, 96, 1, 65536, 1), CFG_N32),        # K >= 64, ungrouped, one view: the concatenated operand on this tile
    ((128, 128, 4, 131072, 2), CFG_N32),     # grouped; two views
    ((64, 64, 1, 65536, 1), CFG_N64),
    ((64, 96, 1, 66048, 1), CFG_N64),        # 129 column tiles in ranges of 3
    ((128, 512, 1, 131072, 1), CFG_N128),
    ((96, 512, 1, 131584, 1), CFG_N128),     # ragged rows; 257 tiles
]
# f32 output (ops.split_gemm_f32: the plan is that of (R, 3 K, 1, M, 1)): K = R, one shape per configuration the plan
# picks for 3 K; the XL-planned one runs on the L tile (the four-wave tile has no f32-output form)
SPLIT_SHAPES = [((64, 64, 256), CFG_S), ((576, 576, 256), CFG_L), ((512, 512, 768), CFG_XL), ((32, 32, 65536), CFG_N32),
                ((64, 64, 65536), CFG_N64), ((128, 128, 524288), CFG_N128)]
# the forms of gemm_run and the tiles that lack one: it runs on the L tile with the plan of XL
FORMS = ("plain", "stats", "pro", "pro_stats", "epi", "cat", "f32")
XL_FALLBACK_FORMS = ("pro", "pro_stats", "epi", "f32")
N128_PRO_MAX_KG = 1024

# weight gradient: tile ids of wgrad.hip (WgTileId); 9 is the register-staged kernel, which is no LDS-DMA tile
WG_TILES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10)
WG_PRO_TILES = (0, 1, 2, 3, 4, 5, 8, 10)      # SG and LG (6, 7) have no normalise-on-load form
WG_CHUNK128_TILES = (8, 10)                   # T128 / S128 fall back to T / S where (M / views) % 128 != 0
# (cout, cin, groups, M, views)
WG_SHAPES = [(96, 160, 1, 448, 1),            # one slice; ragged row and column tiles; (M / views) % 128 != 0
             (96, 160, 1, 1280, 1),           # three slices
             (256, 512, 1, 64, 1),            # one chunk; (M / views) % 128 != 0
             (512, 1024, 4, 1024, 2),         # groups and views
             (320, 256, 1, 4160, 1)]          # nine slices with the last one short; (M / views) % 128 != 0
# the register-staged kernel (plan code -1) and the width of its tile
WG_REG_SHAPES = [((40, 24, 1, 777, 1), 64),   # M not a multiple of 8; short last split
                 ((64, 64, 1, 1001, 1), 64),
                 ((256, 256, 1, 1027, 1), 128),   # the 128 tile; three splits
                 ((64, 96, 2, 1728, 3), 64)]      # cin_g % 32 != 0; grouped
# the f32 route (grafp_conv1x1_wgrad_f32, through ops.conv1x1_rows(...).backward): (cout, cin, groups, M)
WG_F32_SHAPES = [(40, 24, 1, 777), (96, 192, 4, 1001), (64, 64, 1, 1024)]

# name, entry point of grafp_amd.ops, form, shape, expected plan code (GEMM: info[0] of grafp_conv1x1_gemm_plan; weight
# gradient: the forced tile id, -1 the register-staged kernel, None the f32 kernel), arg: the activation code (pro,
# pro_stats, epi, wgrad pro), K1 (cat), "wide_w" / "wide_x" / "wide_g" (the f32 routes: which operand has the low plane)
Case = namedtuple("Case", "name entry form shape plan arg")


def cat_splits(K):
    """K1 of the concatenated-operand cases: 32, K - 32 and a multiple of 32 that is not half of K (what K leaves of them)."""
    mid = (K // 32 * 3 // 8) * 32
    return sorted({k1 for k1 in (32, K - 32, mid) if 0 < k1 < K and (k1 != K // 2 or K == 64)})


def _gemm_cases():
    out = []
    for shape, cfg in GEMM_SHAPES:
        R, K, groups, M, views = shape
        tag = f"{CFG_NAMES[cfg]}-{R}x{K}g{groups}x{M}v{views}"
        out.append(Case(f"{tag}-plain", "conv1x1_gemm", "plain", shape, cfg, None))
        out.append(Case(f"{tag}-stats", "conv1x1_gemm", "stats", shape, cfg, None))
        for act in (ACT_NONE, ACT_RELU, ACT_LEAKY):
            out.append(Case(f"{tag}-pro{act}", "conv1x1_gemm", "pro", shape, cfg, act))
            out.append(Case(f"{tag}-pro{act}-stats", "conv1x1_gemm", "pro_stats", shape, cfg, act))
        for act in (ACT_NONE, ACT_RELU, ACT_LEAKY):
            out.append(Case(f"{tag}-epi{act}", "conv1x1_gemm_affine", "epi", shape, cfg, act))
        if groups == 1 and views == 1:
            for k1 in cat_splits(K):
                out.append(Case(f"{tag}-cat{k1}", "conv1x1_gemm_cat", "cat", shape, cfg, k1))
    for (R, K, M), cfg in SPLIT_SHAPES:
        for wide in ("wide_w", "wide_x"):
            out.append(Case(f"{CFG_NAMES[cfg]}-{R}x{K}x{M}-f32-{wide}", "split_gemm_f32", "f32", (R, K, 1, M, 1), cfg, wide))
    return out


def _wgrad_cases():
    out = []
    for i, shape in enumerate(WG_SHAPES):
        tag = "x".join(str(v) for v in shape)
        for tile in WG_TILES:
            out.append(Case(f"wg-{tag}-t{tile}-plain", "conv1x1_wgrad", "plain", shape, tile, None))
        for tile in WG_PRO_TILES:
            act = ACT_RELU if (i + tile) % 2 == 0 else ACT_LEAKY
            out.append(Case(f"wg-{tag}-t{tile}-pro{act}", "conv1x1_wgrad", "pro", shape, tile, act))
    for shape, _tw in WG_REG_SHAPES:
        out.append(Case("wg-" + "x".join(str(v) for v in shape) + "-reg", "conv1x1_wgrad", "plain", shape, -1, None))
    for shape in WG_F32_SHAPES:
        for wide in ("wide_g", "wide_x"):
            out.append(Case("wg-" + "x".join(str(v) for v in shape) + f"-f32-{wide}", "conv1x1_rows.backward", "f32",
                            shape + (1,), None, wide))
    return out


GEMM_CASES = _gemm_cases()
WGRAD_CASES = _wgrad_cases()
CASES = GEMM_CASES + WGRAD_CASES
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# the cells of the form x tile matrix that the library refuses, with the refusal's reason (tests/test_gemm_exact_cpu.py
# holds CASES against this list: every other cell has a case)
REFUSED = {
    ("cat", "groups > 1 or views > 1"): "grafp_conv1x1_gemm_cat_bf16 takes no groups and no views (its shape check is that of "
                                        "(R, K1 + K2, 1, M, 1))",
    ("f32", "groups > 1 or views > 1"): "grafp_conv1x1_gemm_split_f32 takes no groups and no views",
    ("pro", "N128 with Kg > 1024"): "conv1x1_gemm: normalise-on-load with <= 128 output rows takes at most 1024 operand rows",
    ("wgrad pro", "tiles 6, 7"): "SG and LG have no normalise-on-load form: with a pro_tab the rule's own choice runs",
    ("wgrad pro", "plan code -1"): "conv1x1_wgrad: the normalise-on-load form needs rows per group % 32 == 0 and columns per "
                                   "view % 64 == 0",
}


# ---- operand makers: CPU tensors on the stated grid, a pure function of (name, shape) ------------------------------------
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode("utf-8")))


# (the last few results are kept and SHARED, read-only: the forms of a shape use the same w / x / g, and the largest
#  operand is 134 MB -- whoever wants to change one clones it)
@functools.lru_cache(maxsize=6)
def ints(name, shape, amax=X_MAX, dtype=torch.bfloat16):
    """Integers in [-amax, amax] (an activation operand)."""
    return torch.randint(-amax, amax + 1, tuple(shape), generator=_gen(name), dtype=torch.int16).to(dtype)


@functools.lru_cache(maxsize=6)
def nonzero_ints(name, shape, amax=W_MAX, dtype=torch.bfloat16):
    """Non-zero integers in [-amax, amax] (weights and gradients: every element reaches every output of its row group)."""
    g = _gen(name)
    mag = torch.randint(1, amax + 1, tuple(shape), generator=g, dtype=torch.int16)
    sign = torch.randint(0, 2, tuple(shape), generator=g, dtype=torch.int16) * 2 - 1
    return (mag * sign).to(dtype)


def affine_table(name, rows, views):
    """(rows, views, 2) f32: scale in {+-0.5, +-1, +-2}, integer shift in [-4, 4]; from one view of a row to the next both
    change (the scale index moves by 1 ... 4 of 6, the shift by 1 ... 7 of 9), and they differ from row to row."""
    g = _gen(name)
    v = torch.arange(views)[None, :]
    si = (torch.randint(0, 6, (rows, 1), generator=g) + v * torch.randint(1, 5, (rows, 1), generator=g)) % 6
    sh = (torch.randint(0, 9, (rows, 1), generator=g) + v * torch.randint(1, 8, (rows, 1), generator=g)) % 9 - SHIFT_MAX
    return torch.stack((torch.tensor(SCALES)[si], sh.float()), dim=-1).contiguous()


def wide_max(length, narrow_max):
    """The largest magnitude of the wide operand of a split-bf16 route so that check_grid holds over a contraction of
    `length` against a narrow operand of at most narrow_max: |hi| + |lo| <= (1 + 2^-7) |v|."""
    return min(WIDE_MAX, int((SUM_CAP - 1) / (length * narrow_max * (1.0 + 2.0 ** -7))))


def planes(v):
    """(hi, lo) of the split-bf16 routes in float32: hi = bf16(v), lo = bf16(v - hi)."""
    hi = v.float().to(torch.bfloat16).float()
    return hi, (v.float() - hi).to(torch.bfloat16).float()


def case_operands(case):
    """The CPU operands of a case as a dict: w, x (products) or g, x (weight gradients) in the dtype the entry point is
    handed, and the tables of the form: pro = (tab, act, slope), epi = (tab, act, slope)."""
    R, K, groups, M, views = case.shape
    key = "x".join(str(v) for v in case.shape)
    if case.form == "f32":
        # the left operand: w (R, K) of the product (contraction K), g (cout, M) of the weight gradient (contraction M)
        a, a_shape, length = ("w", (R, K), K) if case.entry == "split_gemm_f32" else ("g", (R, M), M)
        if case.arg == "wide_x":
            left = nonzero_ints(f"ge:{key}.{a}", a_shape, W_MAX, torch.float32)
            x = nonzero_ints(f"ge:{key}.x.wide", (K, M), wide_max(length, W_MAX), torch.float32)
        else:
            left = nonzero_ints(f"ge:{key}.{a}.wide", a_shape, wide_max(length, X_MAX), torch.float32)
            x = ints(f"ge:{key}.x", (K, M), X_MAX, torch.float32)
        return {a: left, "x": x}
    ops = {"x": ints(f"ge:{key}.x", (K, M))}
    if case.entry == "conv1x1_wgrad":
        ops["g"] = nonzero_ints(f"ge:{key}.g", (R, M))
    else:
        ops["w"] = nonzero_ints(f"ge:{key}.w", (R, K // groups))
    if case.form in ("pro", "pro_stats"):
        ops["pro"] = (affine_table(f"ge:{key}.pro", K, views), case.arg, SLOPE)
    if case.form == "epi":
        ops["epi"] = (affine_table(f"ge:{key}.epi", R, views), case.arg, SLOPE)
    return ops


def _act(u, act, slope):
    return torch.relu(u) if act == ACT_RELU else (torch.where(u > 0, u, slope * u) if act == ACT_LEAKY else u)


def _is_bf16(t):
    return bool(torch.equal(t.to(torch.bfloat16).to(t.dtype), t))


def _check_table(tab):
    assert tab.dtype == torch.float32
    scale, shift = tab[..., 0].double(), tab[..., 1].double()
    assert bool(torch.isin(scale, torch.tensor(SCALES, dtype=torch.float64, device=tab.device)).all())
    assert bool((shift == shift.round()).all()) and float(shift.abs().max()) <= SHIFT_MAX


def check_grid(case, operands):
    """What the exactness argument of this file needs of a case's operands, as a CONDITION (not a measurement):
      * every operand is in the dtype the entry point is handed, holds integers only, and a bf16-route operand at most 8
        significant bits (|w|, |g| <= 4 and non-zero, |x| <= 8);
      * a prologue table is on its grid, and for EVERY x of the grid (not only those drawn) act(x * scale + shift) is a
        multiple of 1/8 that bf16 holds -- 17 values per table entry;
      * a split route's planes reconstruct both operands exactly, so the dropped lo * lo term is zero;
      * sum |a| |b| over the whole contraction (all of K; all of M for a weight gradient, the split-K reduction included),
        bounded by contraction length x largest |a| x largest |b| of the operands at hand (for a split route |hi| + |lo|),
        is below 2^22 grid units.
    Works on the device the operands are on.  -> the bound, in grid units."""
    R, K, groups, M, views = case.shape
    wgrad = "g" in operands
    a, x = operands["g" if wgrad else "w"], operands["x"]
    length = M if wgrad else K // groups
    assert a.shape == ((R, M) if wgrad else (R, K // groups)) and x.shape == (K, M)
    for t in (a, x):
        assert bool((t == t.round()).all()), "integers only"
    assert bool((a != 0).all()), "no zero in a weight or a gradient"
    if case.form == "f32":
        assert a.dtype == torch.float32 and x.dtype == torch.float32
        amax = bmax = 0.0
        wide, narrow = (x, a) if case.arg == "wide_x" else (a, x)
        for t, is_wide in ((wide, True), (narrow, False)):
            hi, lo = planes(t)
            assert torch.equal(hi + lo, t), "hi + lo reconstructs the operand"
            assert bool((lo != 0).any()) == is_wide, "the low plane: non-zero in the wide operand only"
            m = float((hi.abs() + lo.abs()).max())
            amax, bmax = (m, bmax) if is_wide else (amax, m)
        assert float(wide.abs().max()) > 256 and float(narrow.abs().max()) <= X_MAX
        bound = length * amax * bmax
    else:
        assert a.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
        assert float(a.abs().max()) <= W_MAX and float(x.abs().max()) <= X_MAX
        amax, bmax, unit = float(a.abs().max()), float(x.abs().max()), 1
        if "pro" in operands:
            tab, act, slope = operands["pro"]
            assert tab.shape == (K, views, 2) and slope == SLOPE
            _check_table(tab)
            grid = torch.arange(-X_MAX, X_MAX + 1, dtype=torch.float64, device=tab.device)
            u = _act(grid * tab[..., 0:1].double() + tab[..., 1:2].double(), act, slope)          # (K, views, 17)
            assert bool((u * PRO_UNIT == (u * PRO_UNIT).round()).all()) and _is_bf16(u)
            bmax, unit = float(u.abs().max()), PRO_UNIT
        bound = length * amax * bmax * unit
    if "epi" in operands:
        tab, act, slope = operands["epi"]
        assert tab.shape == (R, views, 2) and slope == SLOPE
        _check_table(tab)
    assert bound < SUM_CAP, (case.name, bound)
    return bound


# ---- references in float64 ---------------------------------------------------------------------------------------------
def _exact_f32(t):
    assert torch.equal(t.float().double(), t), "the float64 result is not exact in f32"
    return t


def transformed(x, pro, views):
    """act(x * scale + shift) of a prologue, per row and view, in float64; asserted to be a bf16 value."""
    tab, act, slope = pro
    K = x.shape[0]
    t = tab.to(x.device).double().reshape(K, views, 1, 2)
    u = _act(x.double().reshape(K, views, -1) * t[..., 0] + t[..., 1], act, slope).reshape(x.shape)
    assert _is_bf16(u)
    return u


def affine(y, epi, views):
    """The affine epilogue on the ROUNDED product y (bf16): act(y * scale + shift) per row and view, exact in f32, rounded
    to bf16 once more."""
    tab, act, slope = epi
    R = y.shape[0]
    t = tab.to(y.device).double().reshape(R, views, 1, 2)
    z = _act(y.double().reshape(R, views, -1) * t[..., 0] + t[..., 1], act, slope).reshape(y.shape)
    return _exact_f32(z).float().to(torch.bfloat16)


def _blocks(a, b, groups):
    """cat_i a_i @ b_i over the row groups of a (rows) and b (rows), float64."""
    ra, rb = a.shape[0] // groups, b.shape[0] // groups
    return torch.cat([a[i * ra:(i + 1) * ra] @ b[i * rb:(i + 1) * rb] for i in range(groups)], dim=0)


def product(w, x, groups=1, views=1, pro=None, epi=None, device="cpu", out_dtype=torch.bfloat16):
    """y = W f(x) with the grouped block product, [then the affine epilogue on the rounded y], in float64 on `device`:
    exact in f32 (asserted); returned as .float() (out_dtype float32) or rounded once to bf16."""
    wd, xd = w.to(device).double(), x.to(device)
    xd = transformed(xd, pro, views) if pro is not None else xd.double()
    y = _exact_f32(_blocks(wd, xd, groups))
    del xd
    if out_dtype == torch.float32:
        assert epi is None
        return y.float()
    y = y.float().to(torch.bfloat16)
    return affine(y, epi, views) if epi is not None else y


def cat(w, x1, x2, device="cpu"):
    """y = W [x1; x2] rounded once to bf16."""
    return product(w, torch.cat((x1, x2), dim=0), device=device)


def wgrad(g, x, groups=1, views=1, pro=None, device="cpu"):
    """dW = cat_i g_i f(x_i)^T (cout, cin / groups) in float64 on `device`: exact in f32 (asserted), returned as f32."""
    gd, xd = g.to(device).double(), x.to(device)
    xd = transformed(xd, pro, views) if pro is not None else xd.double()
    rg, rx = gd.shape[0] // groups, xd.shape[0] // groups
    dw = torch.cat([gd[i * rg:(i + 1) * rg] @ xd[i * rx:(i + 1) * rx].t() for i in range(groups)], dim=0)
    return _exact_f32(dw).float()


def case_reference(case, operands, device="cpu"):
    """The reference of a case in the dtype of the kernel's output.  (stats forms: the product; their partials are held
    against float64 on that product by the GPU test.)"""
    R, K, groups, M, views = case.shape
    if case.entry in ("conv1x1_wgrad", "conv1x1_rows.backward"):
        return wgrad(operands["g"], operands["x"], groups, views, operands.get("pro"), device)
    if case.form == "cat":
        return cat(operands["w"], operands["x"][:case.arg], operands["x"][case.arg:], device)
    return product(operands["w"], operands["x"], groups, views, operands.get("pro"), operands.get("epi"), device,
                   torch.float32 if case.form == "f32" else torch.bfloat16)
