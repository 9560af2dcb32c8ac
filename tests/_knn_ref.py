"""Float64 reference of the dynamic k-NN graph (grafp_amd/csrc/knn_graph.hip, knn_pre.hip, knn_split.hip), its inputs,
rules and the table of cases that tests/test_knn_cpu.py and tests/test_gpu_knn.py run (TEST INFRASTRUCTURE).  Plain numpy:
nothing here is imported from grafp_amd or torch.

Definition (knngraph.h): xn = x / max(|x|_2 over the channels, 1e-12); d_ij = sq_i - 2 <xn_i, xn_j> + sq_j; the neighbours
of i are the k smallest d_ij in ascending order, ties to the lowest j.  Here all of it in float64; bf16 inputs are widened
first, so the reference sees the values the kernels see.

The bar: tol(C) = 2 (2 C 2^-24 + 5e-7), twice what knn_split.hip's header states for the rounding of ONE f32 distance of the
oracle's chains -- a statement of the contract, not a measurement of the kernels.  Rules on a result idx (B, N, k):
  validity   every query: indices in [0, N), pairwise distinct, and |d64[q, idx[t]] - sorted_d64[q, t]| <= tol(C) per rank t
             (order statistics move by at most the perturbation; a neighbour from outside the true set misses by orders of
             magnitude);
  equality   queries whose first k + 1 float64 distances are pairwise more than tol(C) apart: idx is the float64 stable
             argsort.  Two candidates with IDENTICAL feature columns count as apart as well: every chain of the contract gives
             them the same bits, so the lower index comes first -- which is what the stable argsort says.
Identical columns get identical float64 distances by construction (the distances are computed among the distinct columns
and expanded: a BLAS need not give two equal columns equal bits), so exact ties are exact here.
Un-normalised integer features are exact in f32 and in f64: every query falls under the equality rule or ties exactly.

The tiers of knn_split.hip, in float64 (ds = a query's sorted distances, ds[0] its own): CERTIFIED when the first k gaps all
exceed the band 2 m(C); else LIGHT when ds[k + 1] - ds[k - 1] exceeds it; else HEAVY.  A gap counts as decided when it is
under a tenth of the band or over ten times it."""
import collections
import functools

import numpy as np

from _hashfill import hash_ints, hash_normalish

Case = collections.namedtuple("Case", "C N B pref_f32 pref_bf16 pre what")

# pref_*: grafp_knn_split_preferred_for (the default route of ops.knn_graph takes knn_split.hip); pre: grafp_knn_pre_supported
CASES = [
    Case(32, 128, 3, 1, 1, 0, "smallest supported shape: one chunk (T = 1 < ring depth), one candidate block"),
    Case(96, 384, 3, 1, 1, 0, "C, N not powers of two; W = N < 512; the second column per thread partly used"),
    Case(64, 640, 3, 1, 1, 1, "N >= 512, N % 512 != 0: ragged last range of pass 3b"),
    Case(160, 896, 3, 0, 1, 0, "the same with C not a power of two, and chc < 32"),
    Case(224, 1152, 2, 0, 1, 0, "three ranges, the last one ragged"),
    Case(32, 2048, 2, 1, 1, 0, "11 index bits"),
    Case(32, 4096, 1, 1, 1, 0, "12 index bits, the largest N"),
    Case(992, 128, 3, 0, 0, 0, "the largest supported C"),
]
PRE_CASES = [                                                      # the pre-filter needs C % 64 == 0
    Case(128, 384, 3, 1, 1, 1, "pre-filter: N not a power of two"),
    Case(192, 256, 3, 0, 1, 1, "pre-filter: C not a power of two (three 64-channel chunks)"),
]
UNSUPPORTED = Case(1024, 128, 3, 0, 0, 1, "ks_margin(1024) > 0.9 * 2^-10: the exact-f32 route")
DTYPES = ("f32", "bf16")
K_GPU, K_CPU = (1, 3, 4), (1, 4)
CLUSTER_COLS = np.arange(40, 65)                                   # 25 nodes: two groups of 16, the second partial
PAIR_COLS = (20, 110)
# (C, N) -> suffix of the hash name.  At 128 nodes the 0.04 cap is 5 queries and tol(1024) leaves out 6 on average: the
# first name gave 7 (f32) and 5 (bf16), this one 3 and 5.  The seed was chosen on the float64 reference alone.
SEED = {(1024, 128): ".s2"}
N_ORDER = 10                                                      # sorted prefix kept per query (k <= 8, + 2)


def triple_cols(N):
    return (5, 90, N - 1)                                          # one member in the last column range


def case_id(c):
    return f"{c.C}-{c.N}-{c.B}"


def tol(C):
    return 2.0 * (2.0 * C * 2.0 ** -24 + 5e-7)


def cap(C):
    """The largest share of an unstructured clip's queries the equality rule may leave out (k <= 4)."""
    return 0.10 if C == 992 else 0.04


def band(C, dtype):
    """2 m(C) as knn_split.hip documents it: the split form (f32 inputs) and the raw form (bf16 inputs)."""
    if dtype == "bf16":
        return 2.0 * (2.0 * (1.5 * C * 2.0 ** -23 + 3.0 * 2.0 ** -23) + 2e-6)
    return 2.0 * (2.0 * (1.15e-5 + 3.6e-7 * C) + 2.0 ** -23 * C + 1e-6)


def to_bf16(x):
    """float32 -> the nearest bf16 (ties to even), widened back to float32: what torch's .to(torch.bfloat16) keeps."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def structure_clips(c):
    """clip of the cluster, of the triple, of the pair; the last clip stays plain wherever there is more than one."""
    return (0, 1, 1) if c.B >= 3 else (0, 0, 0)


def plain_clip(c):
    return c.B - 1 if c.B >= 2 else None


def planted(c):
    """(clip, column) of every planted query: cluster members, the triple, the pair."""
    bc, bt, bp = structure_clips(c)
    return [(bc, int(q)) for q in CLUSTER_COLS] + [(bt, q) for q in triple_cols(c.N)] + [(bp, q) for q in PAIR_COLS]


@functools.lru_cache(maxsize=None)
def inputs(c, dtype):
    """x (B, C, N) float32, read-only; for bf16 the widened bf16 values.  Unless the case is UNSUPPORTED (no structure):
    a 25-node cluster of relative width 1e-3 (1e-2 for bf16, whose resolution is 4e-3), one exact triple, one exact pair."""
    x = hash_normalish(f"knn64:{c.C}.{c.N}{SEED.get((c.C, c.N), '')}", (c.B, c.C, c.N)).astype(np.float32)
    if c is not UNSUPPORTED:
        bc, bt, bp = structure_clips(c)
        noise = hash_normalish(f"knn64:cluster.{c.C}.{c.N}", (c.C, len(CLUSTER_COLS)))
        x[bc][:, CLUSTER_COLS] = x[bc][:, CLUSTER_COLS[:1]] + np.float32(1e-2 if dtype == "bf16" else 1e-3) * noise
        t0, t1, t2 = triple_cols(c.N)
        x[bt, :, t1] = x[bt, :, t0]
        x[bt, :, t2] = x[bt, :, t0]
        x[bp, :, PAIR_COLS[1]] = x[bp, :, PAIR_COLS[0]]
    if dtype == "bf16":
        x = to_bf16(x)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def int_inputs(C, N, B):
    """Un-normalised integer features in [-3, 3]: exact in f32 and f64, with genuine ties."""
    x = hash_ints(f"knn64:int.{C}.{N}", (B, C, N), -3, 3).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def heavy_clips():
    """(2, 64, 640): every node identical / one-hot features (exact ties at distance 2): every query is HEAVY."""
    x = np.ones((2, 64, 640), np.float32)
    x[1] = np.eye(64, dtype=np.float32)[:, np.arange(640) % 64]
    x.setflags(write=False)
    return x


# ---- the reference --------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "d ds order same")


def ref_distances(x, normalize=True):
    """(B, N, N) float64 distances of x (B, C, N), and same (B, N): the first column with a column's values."""
    x = np.asarray(x, np.float64)
    B, C, N = x.shape
    d = np.empty((B, N, N), np.float64)
    same = np.empty((B, N), np.int64)
    for b in range(B):
        cols, first, inv = np.unique(x[b].T, axis=0, return_index=True, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        # np.unique sorts the columns: number every group by its first member instead
        firsts = np.full(len(cols), N, np.int64)
        np.minimum.at(firsts, inv, np.arange(N))
        same[b] = firsts[inv]
        u = x[b][:, firsts]                                        # (C, U): one column per group
        if normalize:
            u = u / np.maximum(np.sqrt((u * u).sum(axis=0, keepdims=True)), 1e-12)
        sq = (u * u).sum(axis=0)
        du = sq[:, None] - 2.0 * (u.T @ u) + sq[None, :]
        np.fill_diagonal(du, 0.0)                                  # a node to itself and to its copies
        d[b] = du[inv][:, inv]
    return d, same


def make_ref(x, normalize=True):
    d, same = ref_distances(x, normalize)
    order = np.argsort(d, axis=-1, kind="stable")[..., :N_ORDER]
    ds = np.take_along_axis(d, order, axis=-1)
    for a in (d, ds, order, same):
        a.setflags(write=False)
    return Ref(d, ds, order, same)


@functools.lru_cache(maxsize=2)
def cached_ref(c, dtype):
    """The float64 reference of a case's inputs, shared read-only by the tests of that case (the two last used are kept:
    the largest is 134 MB)."""
    return make_ref(inputs(c, dtype))


def separated(ref, k, bar):
    """(B, N) bool: the first k + 1 sorted distances pairwise more than `bar` apart, identical columns counting as apart."""
    o = ref.order[..., :k + 1]
    gaps = np.diff(ref.ds[..., :k + 1], axis=-1)
    group = ref.same[np.arange(o.shape[0])[:, None, None], o]
    return ((gaps > bar) | (group[..., 1:] == group[..., :-1])).all(axis=-1)


def excluded_share(ref, k, bar, clip):
    return 1.0 - float(separated(ref, k, bar)[clip].mean())


Verdict = collections.namedtuple("Verdict", "ratio in_range distinct mismatches checked")


def judge(idx, ref, C):
    """Both rules on idx (B, N, k); returns the figures, asserts nothing (see check)."""
    idx = np.asarray(idx).astype(np.int64)
    B, N, k = idx.shape
    in_range = bool(((idx >= 0) & (idx < N)).all())
    safe = np.clip(idx, 0, N - 1)
    srt = np.sort(safe, axis=-1)
    distinct = bool((np.diff(srt, axis=-1) != 0).all()) if k > 1 else True
    got = np.take_along_axis(ref.d, safe, axis=-1)
    ratio = float(np.abs(got - ref.ds[..., :k]).max() / tol(C))
    sep = separated(ref, k, tol(C))
    mism = int((idx[sep] != ref.order[..., :k][sep]).any(axis=-1).sum())
    return Verdict(ratio, in_range, distinct, mism, float(sep.mean()))


def check(idx, ref, C, what=""):
    """Asserts both rules; prints the worst error-to-bar ratio and the share of queries the equality rule covers."""
    v = judge(idx, ref, C)
    print(f"knn {what}: worst |d64[idx] - sorted d64| / tol {v.ratio:.3f}; equality rule on {100.0 * v.checked:.2f} % of the "
          f"queries, {v.mismatches} differ")
    assert v.in_range, f"{what}: an index outside [0, N)"
    assert v.distinct, f"{what}: a query lists a neighbour twice"
    assert v.ratio <= 1.0, f"{what}: a listed neighbour misses its rank's distance by {v.ratio:.3g} tol"
    assert v.mismatches == 0, f"{what}: {v.mismatches} well separated queries differ from the float64 argsort"
    return v


def check_exact(idx, ref, what=""):
    """Integer features: idx is the float64 stable argsort for every query."""
    idx = np.asarray(idx).astype(np.int64)
    k = idx.shape[-1]
    bad = int((idx != ref.order[..., :k]).any(axis=-1).sum())
    print(f"knn {what}: {bad} of {idx.shape[0] * idx.shape[1]} queries differ from the float64 stable argsort")
    assert bad == 0, what


# ---- tiers ----------------------------------------------------------------------------------------------------------
def sure_tiers(ref, k, bnd):
    """(uncertified, light, heavy), each (B, N) bool: what a query must be whatever the rounding (decided gaps only)."""
    gaps = np.diff(ref.ds[..., :k + 1], axis=-1)
    wide = ref.ds[..., k + 1] - ref.ds[..., k - 1]
    unc = (gaps < 0.1 * bnd).any(axis=-1)
    return unc, unc & (wide > 10.0 * bnd), wide < 0.1 * bnd


def sure_uncertified_planted(c, dtype, k):
    """How many of the planted queries must be recomputed exactly: a lower bound of the kernels' uncertified count."""
    unc, _, _ = sure_tiers(cached_ref(c, dtype), k, band(c.C, dtype))
    return sum(int(unc[b, q]) for b, q in planted(c))
