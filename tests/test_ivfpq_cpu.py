"""CPU tests of what the IVF-PQ kernel tests stand on (tests/_ivfpq_ref.py): every exact case satisfies the exactness
condition and holds what it claims to hold, oracle/csrc/ivfpq.c equals the float64 references bit for bit on them and
stays within the two derived bars on random rows, and each planted defect of a kernel moves the reference of some case."""
import numpy as np
import pytest

import _ivfpq_ref as ir
from oracle import ivfpq as oq
from oracle import native


def _probe_cases():
    return [ir.probe_case(*p) for p in ir.PROBE_CASES]


# ---- the exactness condition ------------------------------------------------------------------------------------------
def test_check_exact_holds_for_every_case():
    cases = ([ir.assign_case(c.name) for c in ir.ASSIGN_CASES] + [ir.kmeans_case(c.name) for c in ir.KMEANS_CASES]
             + _probe_cases() + [ir.search_case(*s) for s in ir.SEARCH_SHAPES])
    for case in cases:
        b_dist, b_sum = ir.check_exact(case)
        assert 0 < b_dist < ir.EXACT_CAP and 0 < b_sum < ir.EXACT_CAP


def test_check_exact_refuses_what_breaks_the_argument():
    good = ir.assign_case("d100-k200-res")
    for key, value in (("x", 2.0 ** -5), ("x", 2.0), ("base", 1.0), ("cent", 2.0 ** -6), ("cent", 0.5)):
        bad = dict(good)
        bad[key] = good[key].copy()
        bad[key].reshape(-1)[3] = value
        with pytest.raises(AssertionError):
            ir.check_exact(bad)
    wide = dict(ir.probe_case(300, 20, 128))
    wide["q"], wide["cent"] = np.full((9, 1 << 13), -2.0, np.float32), np.full((300, 1 << 13), 0.9375, np.float32)
    with pytest.raises(AssertionError):                       # on the grids, but 8192 squares of 47 steps pass 2^24
        ir.check_exact(wide)


def test_dyadic_is_closed_form_and_on_its_grid():
    a = ir.dyadic("ivfpq:t", (1000,), 2.0 ** -5, 0.5)
    assert np.array_equal(a, ir.dyadic("ivfpq:t", (1000,), 2.0 ** -5, 0.5)) and a.dtype == np.float32
    assert a.min() == -0.5 and a.max() == 0.5 - 2.0 ** -5 and len(np.unique(a)) == 32
    assert np.array_equal(a[:10], ir.dyadic("ivfpq:t", (10,), 2.0 ** -5, 0.5))


# ---- no case is vacuous -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ir.ASSIGN_CASES, ids=lambda c: c.name)
def test_assign_case_holds_what_it_claims(case):
    c = ir.assign_case(case.name)
    d = case.D // case.G
    asg, dmin, cross = ir.ref_assign(c["x"], c["G"], c["cent"], c["base"], c["base_idx"], stats=True)
    assert c["kb"] == ir.tile(d, case.k) == min(case.k, 65536 // (4 * d))
    if case.dups:
        assert case.k % c["kb"] != 0 and case.k > c["kb"]                      # a remainder tile
        tiles = [j // c["kb"] for j in case.dups]
        assert len(set(tiles)) == len(tiles) and case.lone // c["kb"] == case.k // c["kb"]
        assert cross >= 4                                                    # exact ties across LDS tiles
        assert (asg[[0, 1, case.n // 2, case.n - 1], 0] == case.dups[0]).all() and (dmin[[0, 1, case.n // 2, case.n - 1]] == 0).all()
        assert (asg[[2, case.n - 2], 0] == case.lone).all()
        assert (asg[:, 0] >= case.k // c["kb"] * c["kb"]).sum() >= 4           # rows that belong to the remainder tile
    if case.k == 256:
        assert (asg == 255).any(axis=0).all() and (asg[[7, case.n - 1]] == 255).all()     # code 255 in every sub-space
    assert len(np.unique(asg)) > min(case.k, 64) // 2


@pytest.mark.parametrize("case", ir.KMEANS_CASES, ids=lambda c: c.name)
def test_kmeans_case_holds_what_it_claims(case):
    c = ir.kmeans_case(case.name)
    assert c["cnt"].sum(1).tolist() == [case.n] * case.G
    empty = c["cnt"] == 0
    if case.name in ("fewer-rows", "sub-spaces"):
        assert empty.any() and np.array_equal(c["cent1"][empty], c["cent0"][empty])     # an empty cluster keeps its centroid
    if case.name == "fewer-rows":
        assert len(np.unique(c["init"])) == case.n < case.k                  # repeated seeds: the later duplicates are empty
        assert empty[:, case.n:].all()
    if case.n < case.k:                                                      # every row is its own seed: nothing moves
        return
    assert not np.array_equal(c["cent1"][~empty], c["cent0"][~empty])
    # the division is a real one: some quotient is no f32 number before it is rounded
    r =ir.residuals(c["x"], c["G"], c["base"], c["base_idx"])
    s, cnt = ir._cluster_sums(r, c["asg"], case.k, np.ones(case.n, bool))
    with np.errstate(invalid="ignore", divide="ignore"):
        exact = s / cnt[..., None]
    assert (exact[~empty] != c["cent1"][~empty].astype(np.float64)).any()


@pytest.mark.parametrize("nlist,nprobe,d", ir.PROBE_CASES)
def test_probe_case_holds_what_it_claims(nlist, nprobe, d):
    c = ir.probe_case(nlist, nprobe, d)
    assert len(c["pairs"]) == (2 if nlist > 1 else 0)
    for row, (lo, hi) in enumerate(c["pairs"]):          # the pair is at the front of its query, lower list id first
        assert c["probe"][row, 0] == lo and (nprobe < 2 or c["probe"][row, 1] == hi)
    if nprobe == nlist:
        assert all(sorted(p) == list(range(nlist)) for p in c["probe"].tolist())
    q = c["q"].copy()
    q[ir.PROBE_NAN] = np.nan
    with_nan = ir.ref_probe(q, c["cent"], nprobe)
    assert (with_nan[ir.PROBE_NAN[0]] == -1).all() and np.array_equal(np.delete(with_nan, 8, 0), c["probe"][:8])


@pytest.mark.parametrize("d,M", ir.SEARCH_SHAPES)
def test_search_case_holds_what_it_claims(d, M):
    c = ir.search_case(d, M)
    a, codes = c["a"], c["codes"]
    assert np.bincount(a, minlength=ir.SEARCH_NLIST).tolist() == list(ir.SEARCH_LENS)
    assert {0, 1, 255, 256, 257, 513} <= set(ir.SEARCH_LENS) and ir.SEARCH_NLIST >= 8
    # the twins: one centroid, the same codes at interleaved insertion ids, both orders of the two lists
    ta, tb = (np.nonzero(a == t)[0] for t in ir.TWINS)
    assert np.array_equal(c["cent"][ir.TWINS[0]], c["cent"][ir.TWINS[1]])
    assert np.array_equal(codes[ta[0::2]], codes[tb[0::2]]) and np.array_equal(codes[ta[1::2]], codes[tb[1::2]])
    assert (ta[0::2] < tb[0::2]).all() and (tb[1::2] < ta[1::2]).all()
    D1, I1 = ir.search_reference(d, M, 1)
    D4, I4 = ir.search_reference(d, M, 4)
    Dn, In = ir.search_reference(d, M, ir.SEARCH_NLIST)
    # equal estimates with interleaved ids in two lists, in the answer of query 1
    both =(D4[1, :-1] == D4[1, 1:]) & (a[I4[1, :-1]] != a[I4[1, 1:]]) & (I4[1, :-1] >= 0) & (I4[1, 1:] >= 0)
    assert both.sum() >= 4
    # query 0: only empty lists at nprobe 1; 6 candidates, fewer than k, at nprobe 4; everything at nprobe = nlist
    assert ir.ref_probe(c["q"][:1], c["cent"], 4).tolist() == [list(ir.HUB)]
    assert (I1[0] == -1).all() and np.isinf(D1[0]).all()
    assert (I4[0, :6] >= 0).all() and (I4[0, 6:] == -1).all() and np.isinf(D4[0, 6:]).all()
    assert (In >= 0)[:8].all()
    # the rows at a list's edges are the best of their query
    for i, (lst, rows) in ir.EDGE_ROWS.items():
        members = np.nonzero(a == lst)[0]
        assert members[list(rows)].tolist() == I1[i, :len(rows)].tolist(), (i, lst)
        assert ir.ref_probe(c["q"][i:i + 1], c["cent"], 1)[0, 0] == lst
    assert (I1[8] == -1).all()                                                          # the NaN query


# ---- oracle/csrc/ivfpq.c against the float64 references, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("case", ir.ASSIGN_CASES, ids=lambda c: c.name)
def test_c_oracle_assignment_is_the_float64_argmin(case):
    c = ir.assign_case(case.name)
    want = ir.ref_assign(c["x"], c["G"], c["cent"], c["base"], c["base_idx"])
    assert np.array_equal(native.pq_assign(c["x"], c["G"], c["cent"], c["base"], c["base_idx"]), want)


@pytest.mark.parametrize("case", ir.KMEANS_CASES, ids=lambda c: c.name)
def test_c_oracle_kmeans_is_the_exact_lloyd_step(case):
    c = ir.kmeans_case(case.name)
    args = (c["x"], c["G"], c["k"], c["init"])
    assert np.array_equal(native.kmeans(*args, 0, c["base"], c["base_idx"]), c["cent0"])
    assert np.array_equal(native.kmeans(*args, 1, c["base"], c["base_idx"]), c["cent1"])


@pytest.mark.parametrize("nlist,nprobe,d", ir.PROBE_CASES)
def test_c_oracle_probe_is_the_lexsort(nlist, nprobe, d):
    c = ir.probe_case(nlist, nprobe, d)
    assert np.array_equal(native.ivfpq_probe(c["q"], c["cent"], nprobe), c["probe"])


@pytest.mark.parametrize("d,M", ir.SEARCH_SHAPES)
def test_c_oracle_search_and_both_float64_forms_agree(d, M):
    """oracle.ivfpq.search (the reference of the GPU test), ref_search (the form the defects are planted into) and
    oracle/csrc/ivfpq.c: equal ids, equal distances, on the finite queries; the NaN query is the C search's with the
    probe row of -1 that the probe kernel gives it."""
    c = ir.search_case(d, M)
    order, start = ir.list_order(c["a"], ir.SEARCH_NLIST)
    q = c["q"].copy()
    q[ir.SEARCH_NAN] = np.nan
    for nprobe in ir.SEARCH_NPROBE:
        D, I = ir.search_reference(d, M, nprobe)
        D2, I2 = ir.ref_search(q, c["a"], c["codes"], c["cent"], c["books"], nprobe, 50)
        assert np.array_equal(D, D2) and np.array_equal(I, I2)
        probe = ir.ref_probe(q, c["cent"], nprobe)
        assert np.array_equal(native.ivfpq_probe(q[:8], c["cent"], nprobe), probe[:8])
        for k in ir.SEARCH_K_FUSED + ir.SEARCH_K_DENSE:
            Dc, Ic = native.ivfpq_search(q, c["cent"], c["books"], c["codes"][order], start, order, probe, k)
            assert np.array_equal(Ic, I[:, :k]) and np.array_equal(Dc.astype(np.float64), D[:, :k])


# ---- random unit rows: the oracle within the two derived bars ---------------------------------------------------------
def _native_kmeans(x, G, k, niter, seed, base, base_idx):
    return native.kmeans(x, G, k, ir.init_rows(x.shape[0], k, seed), niter, base, base_idx)


@pytest.mark.parametrize("d,M,nlist,n", ir.RANDOM_CASES)
def test_c_oracle_within_both_bars_on_random_rows(d, M, nlist, n):
    x = ir.random_rows(d, n)
    for name, G, k, base, base_idx, seed in ir.random_forms(d, M, nlist, n, _native_kmeans, native.pq_assign):
        prev = _native_kmeans(x, G, k, ir.RANDOM_NITER - 1, seed, base, base_idx)
        last = _native_kmeans(x, G, k, ir.RANDOM_NITER, seed, base, base_idx)
        asg = native.pq_assign(x, G, prev, base, base_idx)
        cert = ir.assign_certificate(x, G, prev, asg, base, base_idx)
        ratio, kept, empty = ir.lloyd_identity(last, prev, x, G, asg, base, base_idx)
        print(f"ivfpq bars, C oracle ({d}, {M}, {nlist}, {n}) {name}: certificate {cert:.3f}, Lloyd {ratio:.3f} of the "
              f"bar, {empty} empty clusters")
        assert cert <= 1.0 and ratio <= 1.0 and kept
        # a dropped row is far outside the Lloyd bar, and a wrong choice outside the certificate
        bad, _, _ = ir.lloyd_identity(last, prev, x, G, asg, base, base_idx, defect="drop_chunk_last_row")
        assert bad > 1.0
        wrong = asg.copy()
        wrong[::7] = (wrong[::7] + 1) % k
        assert ir.assign_certificate(x, G, prev, wrong, base, base_idx) > 1.0


# ---- every planted defect moves the reference of some case -------------------------------------------------------------
def _assign_moves(defect):
    moved = []
    for case in ir.ASSIGN_CASES:
        c = ir.assign_case(case.name)
        args = (c["x"], c["G"], c["cent"], c["base"], c["base_idx"])
        if not np.array_equal(ir.ref_assign(*args, defect=defect), ir.ref_assign(*args)):
            moved.append(case.name)
    return moved


def _search_moves(defect):
    moved = []
    for d, M in ir.SEARCH_SHAPES:
        c = ir.search_case(d, M)
        for nprobe in ir.SEARCH_NPROBE:
            D, I = ir.search_reference(d, M, nprobe)
            D2, I2 = ir.ref_search(c["q"][:8], c["a"], c["codes"], c["cent"], c["books"], nprobe, 50, defect=defect)
            for k in ir.SEARCH_K_FUSED + ir.SEARCH_K_DENSE:
                if not (np.array_equal(I[:8, :k], I2[:, :k]) and np.array_equal(D[:8, :k], D2[:, :k])):
                    moved.append((d, M, nprobe, k))
    return moved


@pytest.mark.parametrize("defect", ir.DEFECTS)
def test_planted_defect_moves_the_reference_of_some_case(defect):
    tiled = {c.name for c in ir.ASSIGN_CASES if c.dups}
    shapes, all_k = set(ir.SEARCH_SHAPES), set(ir.SEARCH_K_FUSED + ir.SEARCH_K_DENSE)
    if defect == "highest_id":
        assert tiled <= set(_assign_moves(defect))                          # ... and the k = 256 cases with equal codewords
    elif defect == "drop_remainder_tile":
        assert set(_assign_moves(defect)) == tiled
    elif defect == "no_residual":
        assert set(_assign_moves(defect)) == {c.name for c in ir.ASSIGN_CASES if c.residual}
    elif defect == "drop_chunk_last_row":         # every k-means case in which a row is not its own cluster
        for case in ir.KMEANS_CASES:
            if case.n < case.k:
                continue
            c = ir.kmeans_case(case.name)
            bad, _ = ir.ref_lloyd(c["x"], c["G"], c["cent0"], c["asg"], c["base"], c["base_idx"], defect=defect)
            assert not np.array_equal(bad, c["cent1"]), case.name
    elif defect == "order_by_position":           # every shape, once both twins are probed
        moved = _search_moves(defect)
        assert {m[:2] for m in moved} == shapes and all(m[2] > 1 for m in moved)
    else:                                         # a list's row 256: every shape, every nprobe, every k
        assert defect == "skip_row_256"
        moved = _search_moves(defect)
        assert {m[:2] for m in moved} == shapes and {m[3] for m in moved} == all_k
        assert {m[2] for m in moved} == set(ir.SEARCH_NPROBE)


# ---- the refusals of the index's constructor (they come before the device is asked for) -----------------------------------
def test_index_refuses_what_the_search_kernel_does_not_serve():
    from grafp_amd.ivfpq import IVFPQIndex
    with pytest.raises(ValueError, match=r"d / M = 3 not in \{1, 2, 4, 8\}"):
        IVFPQIndex(d=24, M=8)
    with pytest.raises(ValueError, match=r"d / M = 16 not in \{1, 2, 4, 8\}"):
        IVFPQIndex(d=128, M=8)
    with pytest.raises(ValueError, match=r"M = 151 sub-quantisers need 154624 bytes of LDS"):
        IVFPQIndex(d=151, M=151)
    with pytest.raises(ValueError, match="multiple of M"):
        IVFPQIndex(d=100, M=64)


def test_float64_assignment_agrees_with_the_published_definition():
    """ref_assign (direct differences) and oracle/ivfpq.py::encode (the expanded form) are the same function on the grid."""
    c = ir.assign_case("d2-res")
    a, codes = oq.encode(c["x"], c["base"], c["cent"])
    assert np.array_equal(a, ir.ref_assign(c["x"], 1, c["base"][None])[:, 0])
    assert np.array_equal(codes, ir.ref_assign(c["x"], 64, c["cent"], c["base"], a).astype(np.uint8))
