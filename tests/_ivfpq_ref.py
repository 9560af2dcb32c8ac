"""Exact inputs, float64 references, case tables and the two derived bars of the IVF-PQ kernel tests (csrc/ivfpq.hip:
pq_assign_kernel, kmeans_*_kernel, ivfpq_probe_kernel, ivfpq_search_kernel, ivfpq_adc_kernel) (TEST INFRASTRUCTURE):
tests/test_ivfpq_cpu.py pins them on the CPU and holds oracle/csrc/ivfpq.c against them, tests/test_gpu_ivfpq.py holds the
kernels against them.  Nothing here needs a GPU.

Exact, because the inputs sit on grids on which every number the kernels form is exact in f32, in ANY summation order:
  * rows and queries: multiples of 2^-4 in [-2, 2); coarse centroids: multiples of 2^-4 in [-1, 1); codewords: multiples of
    2^-5 in [-0.5, 0.5);
  * a residual x - centroid is a multiple of 2^-4 below 3, a difference to a codeword a multiple of 2^-5 below 3.5, its
    square a multiple of 2^-10 below 12.25: a sum of d of them (one distance), of all M d/M of them (one ADC estimate), in
    units of the square of the grid step, is an integer below 2^24 (check_exact) -- an fmaf chain, a plain sum and the
    float64 sum give the same number, so argmin and the (estimate, id) order are defined by float64 alone;
  * a cluster sum of n residuals is an integer number of 2^-4 steps below 2^24 as well: the 1024-row chunks, the chunk
    order and the row order do not show, and one Lloyd step is the exact sum and ONE f32 division.
On random unit rows nothing is exact; there the two bars at the end of this file hold, both derived with u = 2^-24."""
import functools
from collections import namedtuple

import numpy as np

from _hashfill import hash_ints, hash_normalish, hash_uniform

U = 2.0 ** -24
KM_CHUNK = 1024                     # rows per partial sum of kmeans_partial_kernel
LDS_TILE_BYTES = 64 * 1024          # pq_assign_kernel: centroids per LDS tile = 65536 / (4 d)
EXACT_CAP = 1 << 24
ROW_GRID, CENT_GRID, WORD_GRID = (2.0 ** -4, 2.0), (2.0 ** -4, 1.0), (2.0 ** -5, 0.5)      # (step, limit)
DEFECTS = ("highest_id", "drop_remainder_tile", "no_residual", "drop_chunk_last_row", "order_by_position", "skip_row_256")


def dyadic(tag, shape, step, lim):
    """f32 multiples of `step` in [-lim, lim), a pure function of (tag, index) (no RNG state)."""
    levels = int(round(2 * lim / step))
    return ((hash_ints(tag, shape, 0, levels - 1).astype(np.float64) - levels // 2) * step).astype(np.float32)


def tile(d, k):
    """kb of grafp_pq_assign_f32: the centroids of a sub-space pass through LDS kb at a time."""
    return min(k, LDS_TILE_BYTES // (4 * d))


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _on_grid(a, grid):
    step, lim = grid
    a = np.asarray(a, dtype=np.float64)
    return bool((a / step == np.round(a / step)).all() and (a >= -lim).all() and (a < lim).all())


# ---- float64 references ------------------------------------------------------------------------------------------------
def residuals(x, G, base=None, base_idx=None, defect=None):
    """(n, G, d) float64: x[row] - base[base_idx[row]] (exact in float64 for f32 inputs), split into G sub-spaces."""
    r = np.asarray(x, dtype=np.float64)
    if base is not None and defect != "no_residual":
        r = r - np.asarray(base, dtype=np.float64)[np.asarray(base_idx)]
    return r.reshape(r.shape[0], G, -1)


def _nearest(r, c):
    """r (n, d), c (k, d) float64 -> (lowest argmin, highest argmin, minimum) of the direct sum over c of (r - c)^2."""
    n, k = r.shape[0], c.shape[0]
    first, last, dmin = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n)
    step = max(1, (1 << 22) // (k * r.shape[1]))
    for lo in range(0, n, step):
        diff = r[lo:lo + step, None, :] - c[None]
        dist = (diff * diff).sum(-1)
        first[lo:lo + step] = dist.argmin(1)
        last[lo:lo + step] = k - 1 - dist[:, ::-1].argmin(1)
        dmin[lo:lo + step] = dist.min(1)
    return first, last, dmin


def ref_assign(x, G, cent, base=None, base_idx=None, defect=None, stats=False):
    """Nearest centroid of every (row, sub-space): direct sum of (r - c)^2 in float64, np.argmin (lowest id on ties)
    -> (n, G) int32.  stats: also the minimum (n, G) and the number of (row, sub-space) whose minimum is reached in two
    different LDS tiles of pq_assign_kernel."""
    cent = np.asarray(cent, dtype=np.float64)
    r = residuals(x, G, base, base_idx, defect)
    k, d = cent.shape[1], cent.shape[2]
    kb = tile(d, k)
    kk = max(kb, k // kb * kb) if defect == "drop_remainder_tile" else k
    out, dmin, cross = np.empty(r.shape[:2], np.int32), np.empty(r.shape[:2]), 0
    for g in range(G):
        first, last, dmin[:, g] = _nearest(r[:, g], cent[g, :kk])
        out[:, g] = last if defect == "highest_id" else first
        cross += int((first // kb != last // kb).sum())
    return (out, dmin, cross) if stats else out


def _cluster_sums(r, asg, k, keep):
    """sums (G, k, d) and counts (G, k) of the rows `keep` by cluster, float64."""
    n, G, d = r.shape
    s, cnt = np.zeros((G, k, d)), np.zeros((G, k), np.int64)
    for g in range(G):
        np.add.at(s[g], asg[keep, g], r[keep, g])
        cnt[g] = np.bincount(asg[keep, g], minlength=k)
    return s, cnt


def _keep(n, defect):
    keep = np.ones(n, bool)
    if defect == "drop_chunk_last_row":
        keep[KM_CHUNK - 1::KM_CHUNK] = False
        keep[n - 1] = False
    return keep


def ref_lloyd(x, G, prev, asg, base=None, base_idx=None, defect=None, exact=True):
    """One Lloyd update from the assignment `asg` (n, G): the exact cluster sums (asserted to be f32 numbers when
    `exact`), then one f32 division np.float32(s) / np.float32(cnt); an empty cluster keeps `prev`.  -> ((G, k, d) f32,
    counts (G, k))."""
    prev = np.asarray(prev, dtype=np.float32)
    r = residuals(x, G, base, base_idx)
    s, cnt = _cluster_sums(r, np.asarray(asg), prev.shape[1], _keep(r.shape[0], defect))
    if exact:
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s), "a cluster sum is not exact in f32"
    with np.errstate(invalid="ignore", divide="ignore"):
        new = s.astype(np.float32) / cnt.astype(np.float32)[..., None]
    return np.where(cnt[..., None] > 0, new, prev).astype(np.float32), cnt


def ref_probe(q, cent, nprobe):
    """The nprobe nearest lists by np.lexsort((list, dist)), dist the direct float64 sum; a row with a NaN: all -1."""
    q, cent = np.asarray(q, dtype=np.float64), np.asarray(cent, dtype=np.float64)
    out = np.full((q.shape[0], nprobe), -1, np.int32)
    lists = np.arange(cent.shape[0])
    for i in range(q.shape[0]):
        if np.isnan(q[i]).any():
            continue
        diff = q[i][None] - cent
        out[i] = np.lexsort((lists, (diff * diff).sum(1)))[:nprobe]
    return out


def ref_search(q, a, codes, cent, books, nprobe, k, defect=None):
    """The k best candidates of the probed lists by (ADC estimate, insertion id), all in float64; (+inf, -1) where fewer
    exist.  The definition of oracle/ivfpq.py::search written a second time, so that a planted defect can be applied to
    it (tests/test_ivfpq_cpu.py holds the two equal)."""
    M = books.shape[0]
    b64 = np.asarray(books, dtype=np.float64)
    probe = ref_probe(q, cent, nprobe)
    D, I = np.full((len(q), k), np.inf), np.full((len(q), k), -1, np.int64)
    for i in range(len(q)):
        cd, ci = [np.zeros(0)], [np.zeros(0, np.int64)]
        for lst in probe[i]:
            members = np.nonzero(a == lst)[0] if lst >= 0 else np.zeros(0, np.int64)
            if defect == "skip_row_256" and members.size > 256:
                members = np.delete(members, 256)
            if members.size == 0:
                continue
            r = (np.asarray(q[i], dtype=np.float64) - np.asarray(cent[lst], dtype=np.float64)).reshape(M, 1, -1)
            tab = ((r - b64) ** 2).sum(-1)                                                   # (M, 256)
            cd.append(tab[np.arange(M)[None, :], codes[members]].sum(1))
            ci.append(members)
        cd, ci = np.concatenate(cd), np.concatenate(ci)
        order = np.lexsort((np.arange(ci.size) if defect == "order_by_position" else ci, cd))[:k]
        D[i, :order.size], I[i, :order.size] = cd[order], ci[order]
    return D, I


def list_order(a, nlist):
    """What the search kernels are handed: (order (n) position -> insertion id, list_start (nlist + 1))."""
    a = np.asarray(a)
    return np.argsort(a, kind="stable"), np.r_[0, np.cumsum(np.bincount(a, minlength=nlist))].astype(np.int64)


def init_rows(n, k, seed):
    """The documented seeds of grafp_amd.ivfpq.kmeans."""
    from grafp_amd.ivfpq import kmeans_init_rows
    return kmeans_init_rows(n, k, seed).numpy()


# ---- what the exactness argument needs, as a condition --------------------------------------------------------------------
def check_exact(case):
    """Asserts of a case of this file: every input on its grid, and, from the largest magnitudes the inputs at hand can
    form (analytic: no drawn sum can exceed them), in units of the grid step,
      terms x (largest difference)^2 < 2^24   -- terms: the d addends of a distance, all of D for an ADC estimate;
      n x largest |residual| < 2^24           -- a cluster sum over all n rows.
    -> (the two bounds)."""
    kind = case["kind"]
    pts = case["q"] if kind in ("probe", "search") else case["x"]
    assert pts.dtype == np.float32 and _on_grid(pts, ROW_GRID), "rows / queries: multiples of 2^-4 in [-2, 2)"
    max_r, unit = float(np.abs(pts).max()) if pts.size else 0.0, ROW_GRID[0]
    coarse = case["cent"] if kind in ("probe", "search") else case.get("base")
    if coarse is not None:
        assert coarse.dtype == np.float32 and _on_grid(coarse, CENT_GRID), "coarse centroids: multiples of 2^-4 in [-1, 1)"
        max_r += float(np.abs(coarse).max())
    if kind == "kmeans":                                  # the centroids of the checked step are residuals themselves
        max_diff, terms = 2.0 * max_r, case["x"].shape[1] // case["G"]
    elif kind == "probe":
        max_diff, terms = max_r, pts.shape[1]
    else:
        words = case["books"] if kind == "search" else case["cent"]
        grid = CENT_GRID if (kind == "assign" and case["base"] is None) else WORD_GRID
        assert words.dtype == np.float32 and _on_grid(words, grid), "centroids / codewords off their grid"
        max_diff, unit = max_r + float(np.abs(words).max()), grid[0]
        terms = pts.shape[1] if kind == "search" else words.shape[-1]
    b_dist = terms * (max_diff / unit) ** 2
    b_sum = pts.shape[0] * max_r / ROW_GRID[0]
    assert b_dist < EXACT_CAP and b_sum < EXACT_CAP, (b_dist, b_sum)
    return b_dist, b_sum


# ---- pq_assign: the exact cases -------------------------------------------------------------------------------------------
# dups: centroid ids made equal (members in different LDS tiles), with four rows at distance 0 of all of them; lone: a
# centroid of the remainder tile with two rows at distance 0 of it alone
AssignCase = namedtuple("AssignCase", "name D G k n residual dups lone")
ASSIGN_CASES = [
    AssignCase("d128-k300", 128, 1, 300, 513, False, (5, 133, 290), 295),      # tiles 128 + 128 + 44
    AssignCase("d100-k200-res", 100, 1, 200, 257, True, (10, 180), 190),       # kb = 163: tiles 163 + 37; d below DCAP
    AssignCase("d33-k512", 33, 1, 512, 256, False, (2, 500), 505),             # kb = 496: tiles 496 + 16
    AssignCase("d32-k7", 32, 1, 7, 255, False, (), None),                      # DCAP 32 edge
    AssignCase("d9-res", 36, 4, 256, 300, True, (), None),
    AssignCase("d3-res", 6, 2, 256, 300, True, (), None),
    AssignCase("d2-res", 128, 64, 256, 300, True, (), None),
    AssignCase("d1-res", 128, 128, 256, 300, True, (), None),
]
ASSIGN_BY_NAME = {c.name: c for c in ASSIGN_CASES}
CORNER = WORD_GRID[1] - WORD_GRID[0]               # 15/32: the largest codeword coordinate


@functools.lru_cache(maxsize=None)
def assign_case(name):
    """x (n, D), cent (G, k, d), base (5, D) / base_idx (n) or None, read-only.  Cases with k = 256 reach code 255: its
    codeword is the corner (15/32, ...), which no other codeword equals, and rows 7 and n - 1 lie beyond it in every
    sub-space."""
    c = ASSIGN_BY_NAME[name]
    d, tag = c.D // c.G, f"ivfpq:assign:{name}"
    x = dyadic(f"{tag}.x", (c.n, c.D), *ROW_GRID)
    base = base_idx = None
    if c.residual:
        base = dyadic(f"{tag}.base", (5, c.D), *CENT_GRID)
        base_idx = hash_ints(f"{tag}.bi", (c.n,), 0, 4).astype(np.int32)
    cent = dyadic(f"{tag}.cent", (c.G, c.k, d), *(WORD_GRID if c.residual else CENT_GRID))
    offset = (lambda rows: base[base_idx[rows]]) if c.residual else (lambda rows: 0.0)
    if c.dups:
        step = ROW_GRID[0]                         # the planted centroids: on the row grid, so that base + centroid is a row
        for j in (c.dups[0], c.lone):
            cent[0, j] = np.floor(cent[0, j] / step) * step
        cent[0, list(c.dups[1:])] = cent[0, c.dups[0]]
        for rows, j in (([0, 1, c.n // 2, c.n - 1], c.dups[0]), ([2, c.n - 2], c.lone)):
            x[rows] = offset(rows) + cent[0, j]
    if c.k == 256:
        first = cent[:, :255, 0]
        first[first == CORNER] = -WORD_GRID[1]
        cent[:, 255, :] = CORNER
        x[[7, c.n - 1]] = ROW_GRID[1] - ROW_GRID[0]
    return _frozen({"kind": "assign", "x": x, "cent": cent, "base": base, "base_idx": base_idx, "G": c.G, "kb": tile(d, c.k)})


# ---- k-means: the exact cases ---------------------------------------------------------------------------------------------
KmeansCase = namedtuple("KmeansCase", "name D G k n residual")
KMEANS_CASES = [KmeansCase(f"n{n}", 32, 1, 16, n, False) for n in (1023, 1024, 1025, 2049)] + [   # around KM_CHUNK
    KmeansCase("fewer-rows", 32, 8, 256, 100, True),        # repeated seeds: the later duplicates stay empty
    KmeansCase("tiled", 128, 1, 300, 1500, False),          # the tiled assignment inside the loop
    KmeansCase("sub-spaces", 32, 16, 256, 1500, True),
]
KMEANS_BY_NAME = {c.name: c for c in KMEANS_CASES}
KMEANS_SEED = 1234


@functools.lru_cache(maxsize=None)
def kmeans_case(name):
    """x, base / base_idx, the seeds' residuals cent0 (niter 0), the exact assignment to them and the exact Lloyd step
    cent1 (niter 1) with the cluster counts."""
    c = KMEANS_BY_NAME[name]
    tag = f"ivfpq:kmeans:{name}"
    x = dyadic(f"{tag}.x", (c.n, c.D), *ROW_GRID)
    base = base_idx = None
    if c.residual:
        base = dyadic(f"{tag}.base", (4, c.D), *CENT_GRID)
        base_idx = hash_ints(f"{tag}.bi", (c.n,), 0, 3).astype(np.int32)
    init = init_rows(c.n, c.k, KMEANS_SEED)
    cent0 = np.ascontiguousarray(residuals(x, c.G, base, base_idx)[init].transpose(1, 0, 2)).astype(np.float32)
    asg = ref_assign(x, c.G, cent0, base, base_idx)
    cent1, cnt = ref_lloyd(x, c.G, cent0, asg, base, base_idx)
    return _frozen({"kind": "kmeans", "x": x, "base": base, "base_idx": base_idx, "G": c.G, "k": c.k, "init": init,
                    "cent0": cent0, "asg": asg, "cent1": cent1, "cnt": cnt})


# ---- probe: the exact cases -------------------------------------------------------------------------------------------
PROBE_CASES = [(1, 1, 32), (63, 63, 32), (64, 5, 32), (65, 65, 32), (130, 20, 32), (300, 20, 128)]    # (nlist, nprobe, d)
PROBE_NAN = (8, 3)                      # the test puts a NaN here; q itself is finite


def probe_pairs(nlist):
    """Two pairs of equal centroids (none at nlist = 1): the first and the last list -- at 65 lists both on lane 0 of the
    wave -- and two in the middle."""
    return ((0, nlist - 1), (2, nlist // 2 + 1)) if nlist >= 6 else ()


@functools.lru_cache(maxsize=None)
def probe_case(nlist, nprobe, d):
    """9 queries: row 0 is a duplicated centroid (a tie at the front), row 1 sits beside the other pair."""
    tag = f"ivfpq:probe:{nlist}.{d}"
    cent = dyadic(f"{tag}.cent", (nlist, d), *CENT_GRID)
    q = dyadic(f"{tag}.q", (9, d), *ROW_GRID)
    pairs = probe_pairs(nlist)
    for lo, hi in pairs:
        cent[hi] = cent[lo]
    if pairs:
        q[0] = cent[pairs[0][0]]
        q[1] = cent[pairs[1][0]] + dyadic(f"{tag}.q1", (d,), 2.0 ** -4, 0.125)
    return _frozen({"kind": "probe", "q": q, "cent": cent, "pairs": pairs, "probe": ref_probe(q, cent, nprobe)})


# ---- fused search and dense scan: the exact cases ---------------------------------------------------------------------
SEARCH_SHAPES = [(128, 64), (128, 128), (64, 16), (32, 8), (96, 12), (24, 24)]           # (d, M)
SEARCH_LENS = (257, 0, 1, 255, 256, 513, 40, 40, 0, 5)                                   # rows of list 0 ... 9
SEARCH_NLIST = len(SEARCH_LENS)
TWINS = (6, 7)                  # one centroid, the same codes, interleaved insertion ids
HUB = (8, 1, 2, 9)              # query 0 is centroid 8; 1, 2 and 9 are its nearest: 0 + 0 + 1 + 5 rows
# query -> (list it is aimed at, rows of that list that hold the query's own best codes): the rows at a list's edges
EDGE_ROWS = {2: (0, (256,)), 3: (5, (256, 512)), 4: (4, (255,)), 5: (3, (254,)), 6: (2, (0,))}
SEARCH_NPROBE = (1, 4, SEARCH_NLIST)
SEARCH_K_FUSED, SEARCH_K_DENSE = (1, 20, 32), (33, 50)
SEARCH_NAN = (8, 3)


@functools.lru_cache(maxsize=None)
def search_case(d, M):
    """q (9, d): row 0 = centroid 8 (its list is empty: nprobe 1 finds nothing, nprobe 4 finds 6 rows), row 1 beside
    the twins' centroid, rows 2-6 beside the centroids of EDGE_ROWS, rows 7-8 anywhere (the test puts a NaN into row 8).
    a (n) list ids and codes (n, M) in insertion order (hand-built: a closed-form shuffle of SEARCH_LENS)."""
    tag = f"ivfpq:search:{d}.{M}"
    nlist, n = SEARCH_NLIST, sum(SEARCH_LENS)
    cent = dyadic(f"{tag}.cent", (nlist, d), *CENT_GRID)
    books = dyadic(f"{tag}.books", (M, 256, d // M), *WORD_GRID)
    cent[TWINS[1]] = cent[TWINS[0]]
    for t, lst in enumerate(HUB[1:]):             # one coordinate away from centroid 8, by 1, 2, 3 grid steps
        cent[lst] = cent[HUB[0]]
        delta = (t + 1) * CENT_GRID[0]
        cent[lst, t] += delta if cent[lst, t] + delta < CENT_GRID[1] else -delta
    a = np.repeat(np.arange(nlist), SEARCH_LENS)[np.argsort(hash_uniform(f"{tag}.order", (n,)), kind="stable")]
    a = a.astype(np.int32)
    codes = hash_ints(f"{tag}.codes", (n, M), 0, 255).astype(np.uint8)
    tw = np.nonzero((a == TWINS[0]) | (a == TWINS[1]))[0]
    a[tw] = np.array([TWINS[0], TWINS[1], TWINS[1], TWINS[0]], np.int32)[np.arange(tw.size) % 4]
    codes[tw] = codes[tw[np.arange(tw.size) // 4 * 4]]       # four consecutive twin rows share their codes
    q = dyadic(f"{tag}.q", (9, d), *ROW_GRID)
    near = dyadic(f"{tag}.near", (9, d), 2.0 ** -4, 0.5)
    q[0] = cent[HUB[0]]
    q[1] = cent[TWINS[0]] + near[1]
    for i, (lst, rows) in EDGE_ROWS.items():
        if lst in HUB:                            # the hub's centroids differ in coordinates 0 ... 2 only: stay on `lst` there
            near[i, :len(HUB) - 1] = 0.0
        q[i] = cent[lst] + near[i]
        best = ref_assign(q[i][None], M, books, cent, np.array([lst])).astype(np.uint8)
        codes[np.nonzero(a == lst)[0][list(rows)]] = best
    return _frozen({"kind": "search", "q": q, "cent": cent, "books": books, "a": a, "codes": codes})


@functools.lru_cache(maxsize=None)
def search_reference(d, M, nprobe):
    """oracle.ivfpq.search at k = 50 (its first k columns are the result for a smaller k) on the finite queries, with
    the row of the NaN query appended: a query with a NaN probes no list, (+inf, -1)."""
    from oracle import ivfpq as oq
    c = search_case(d, M)
    D, I = oq.search(c["q"][:SEARCH_NAN[0]], c["a"], c["codes"], c["cent"], c["books"], nprobe, max(SEARCH_K_DENSE))
    D, I = np.vstack([D, np.full((1, D.shape[1]), np.inf)]), np.vstack([I, np.full((1, I.shape[1]), -1, np.int64)])
    D.setflags(write=False), I.setflags(write=False)
    return D, I


# ---- random unit rows: nothing is exact, two derived bars ---------------------------------------------------------------
RANDOM_CASES = [(128, 64, 16, 3000), (32, 8, 5, 2500), (96, 12, 7, 2100)]                # (d, M, nlist, n)
RANDOM_NITER = 3


@functools.lru_cache(maxsize=None)
def random_rows(d, n):
    x = hash_normalish(f"ivfpq:random:{d}.{n}", (n, d)).astype(np.float64)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    x.setflags(write=False)
    return x


def random_forms(d, M, nlist, n, kmeans, assign):
    """The two k-means of an index over the random rows, as (name, G, k, base, base_idx, seed): the coarse one, and the
    codebooks' on the residuals to ITS result (RANDOM_NITER iterations of `kmeans`, assigned by `assign`).
    kmeans(x, G, k, niter, seed, base, base_idx) -> (G, k, d); assign(x, G, cent, base, base_idx) -> (n, G)."""
    x = random_rows(d, n)
    yield "coarse", 1, nlist, None, None, KMEANS_SEED
    cent = np.ascontiguousarray(kmeans(x, 1, nlist, RANDOM_NITER, KMEANS_SEED, None, None)[0])
    yield "codebooks", M, 256, cent, np.ascontiguousarray(assign(x, 1, cent[None], None, None)[:, 0]), KMEANS_SEED + 2


def assign_certificate(x, G, cent, asg, base=None, base_idx=None):
    """Largest (D - D*) / bound over the (row, sub-space): D the float64 distance to the chosen centroid, D* the float64
    minimum, R = sum r^2, bound = u [(d + 4)(D + D*) + 2 (sqrt(D R) + sqrt(D* R))].
    Why: the kernel chose j because its f32 value of D_j was not above its value of D*.  An fmaf chain of d squares of
    rounded differences is off by at most (d + 2) u D (d - 1 additions and the two roundings of a term, to first order;
    the bar has d + 4), and the ONE rounding of the residual, |dr| <= u |r|, moves a distance by at most
    2 sqrt(D) u sqrt(R).  A value of at most 1 is a certificate that the choice is a float64 argmin within f32's reach."""
    cent = np.asarray(cent, dtype=np.float64)
    r = residuals(x, G, base, base_idx)
    d, worst = cent.shape[2], 0.0
    for g in range(G):
        _, _, dstar = _nearest(r[:, g], cent[g])
        diff = r[:, g] - cent[g][np.asarray(asg)[:, g]]
        D, R = (diff * diff).sum(1), (r[:, g] * r[:, g]).sum(1)
        bound = U * ((d + 4) * (D + dstar) + 2.0 * (np.sqrt(D * R) + np.sqrt(dstar * R)))
        gap = D - dstar
        assert (gap >= 0).all()
        ratio = np.divide(gap, bound, out=np.zeros_like(gap), where=gap > 0)
        worst = max(worst, float(ratio.max()))
    return worst


def lloyd_identity(c_t, c_prev, x, G, asg, base=None, base_idx=None, defect=None):
    """The Lloyd-step identity of c_t = kmeans(niter t) given c_prev = kmeans(niter t - 1) and asg = the assignment to
    c_prev: per coordinate of a non-empty cluster |c_t - mean64| <= (min(cnt, 1024) + nchunks + 2) u sum|v| / cnt -- a
    chunk adds at most min(cnt, 1024) residuals one after the other, the chunk sums are added nchunks at a time, every
    residual is rounded once and the quotient once, 2 for the second order -- and an empty cluster keeps c_prev bit for
    bit.  -> (largest error / bar, whether every empty cluster kept its centroid, number of empty clusters).
    defect: applied to c_t's stand-in, the float64 mean (tests/test_ivfpq_cpu.py: a dropped row is far outside)."""
    c_t, c_prev = np.asarray(c_t, dtype=np.float32), np.asarray(c_prev, dtype=np.float32)
    r = residuals(x, G, base, base_idx)
    n, k = r.shape[0], c_prev.shape[1]
    keep = np.ones(n, bool)
    s, cnt = _cluster_sums(r, np.asarray(asg), k, keep)
    sabs, _ = _cluster_sums(np.abs(r), np.asarray(asg), k, keep)
    if defect is not None:
        sd, cd = _cluster_sums(r, np.asarray(asg), k, _keep(n, defect))
        c_t = np.where(cd[..., None] > 0, sd / np.maximum(cd, 1)[..., None], c_prev).astype(np.float32)
    live = cnt > 0
    nchunks = (n + KM_CHUNK - 1) // KM_CHUNK
    safe = np.maximum(cnt, 1)[..., None]
    bar = (np.minimum(cnt, KM_CHUNK) + nchunks + 2)[..., None] * U * sabs / safe
    err = np.abs(c_t.astype(np.float64) - s / safe)
    ratio = np.divide(err, bar, out=np.where(err > 0, np.inf, 0.0), where=bar > 0)[live]
    kept = bool(np.array_equal(c_t[~live], c_prev[~live]))
    return (float(ratio.max()) if ratio.size else 0.0), kept, int((~live).sum())
