"""CPU tests of the sequence rerank's and the top-k merge's references and case table (tests/_rerank_ref.py): what every
case promises about its own inputs (ties present, unique-candidate counts, the ambiguous share of the real-valued
cases, computed from float64 alone), the sharded reference against the unsharded one, and the C restatements
(oracle/csrc/seq_rerank.c, oracle_merge_topk) over the whole table -- the same table tests/test_gpu_rerank.py runs through
the HIP kernels.  No GPU call is made."""
import numpy as np
import pytest

import _rerank_ref as rr
from oracle import native


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (what, "ids", np.argwhere(got[0] != want[0])[:5])
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, "scores", np.argwhere(_bits(got[1]) != _bits(want[1]))[:5])


def _c_rerank(c, top):
    lens = c["item_len"] if c["max_len"] is None else np.minimum(c["item_len"], c["max_len"])    # the C entry has no clamp
    return native.seq_rerank(c["index"], c["q"], c["ids"], c["item_row"], lens, top=top)


@pytest.mark.parametrize("name", rr.RERANK_CASES)
def test_seq_rerank_c_restatement_over_the_case_table(name):
    """Lattice cases: ids and score bits of oracle/csrc/seq_rerank.c equal the float64-exact reference, ties included,
    and every case marked for ties shows at least one adjacent pair of equal scores in the reference's lists.  Real-valued
    cases: every score within (4m + 6) * 2^-24 * sum|q*x| / m of float64, ids equal outside runs of scores closer than
    their bars, and at most 1 % of the output positions inside such runs."""
    c = rr.rerank_case(name)
    if c["ties"]:
        top = max(c["tops"])
        ties = rr.tie_count(*rr.rerank_want(name, top))
        print(f"{name}: {ties} adjacent equal scores at top {top}")
        assert ties > 0
    if "unique" in c:
        cand = [int((row >= 0).sum()) for row in rr.rerank_want(name, 64)[0]]
        full = rr._spans(c["index"], c["q"], c["ids"], c["item_row"], c["item_len"], None, None)
        assert [len(s[0]) for s in full] == c["unique"] and cand == [min(u, 64) for u in c["unique"]]
    for top in c["tops"]:
        got = _c_rerank(c, top)
        if c["kind"] == "lattice":
            _same(got, rr.rerank_want(name, top), (name, top))
        else:
            args = (c["index"], c["q"], c["ids"], c["item_row"], c["item_len"], top)
            amb, filled = rr.ambiguity(*args, max_len=c["max_len"])
            worst, amb2, filled2 = rr.check_real(got[0], got[1], *args, max_len=c["max_len"])
            print(f"{name} top {top}: worst score deviation {worst:.3f} of its bar, {amb} of {filled} positions ambiguous")
            assert (amb, filled) == (amb2, filled2) and filled > 0 and amb <= 0.01 * filled


def test_case_table_reaches_the_sizes_it_names():
    """ql*k of 1, 63, 64, 65, 1024, 1025 and 2048 (as 64 x 32, as 1 x 2048; 64 x 1), m below ql down to 1 at n - 1, an
    item of zero segments, item_len above max_len, 600 items."""
    counts, min_m, zero_len = set(), {}, False
    for name in rr.RERANK_CASES:
        c = rr.rerank_case(name)
        ql = c["item_len"] if c["max_len"] is None else np.minimum(c["item_len"], c["max_len"])
        counts |= {(int(L), c["k"]) for L in ql}
        zero_len |= bool((ql == 0).any()) and bool((ql > 0).any())
    prod = {L * k for L, k in counts}
    assert {1, 63, 64, 65, 1024, 1025, 2048} <= prod and {(64, 32), (1, 2048), (64, 1)} <= counts and zero_len
    c = rr.rerank_case("lattice_k6")
    spans = rr._spans(c["index"], c["q"], c["ids"], c["item_row"], c["item_len"], None, None)
    cid, m, _s, _a = spans[3]                                       # 19 segments, hits n-1 ... n-6 at segment 0
    assert {1, 2, 3, 4, 5, 6} <= set(m[cid >= c["n"] - 6].tolist()) and int(c["item_len"][3]) == 19
    c = rr.rerank_case("lattice_clamp")
    assert int(c["item_len"].max()) > c["max_len"]
    assert len(rr.rerank_case("lattice_600items")["item_row"]) == 600
    neg = rr.rerank_want("lattice_negative", 10)[1]
    assert (neg[0][np.isfinite(neg[0])] < 0).all() and (neg > 0).any() and (neg[np.isfinite(neg)] < 0).any()


@pytest.mark.parametrize("top", rr.rerank_case(rr.SHARD_CASE)["tops"])
def test_sharded_reference_equals_unsharded_reference(top):
    """Cut into 3 shards, and into 5 of which one is shorter than max_len - 1: per-shard lists merged by the rule of
    ShardedFlatL2Index.rerank equal the one-index result bit for bit; runs that straddle a boundary are found by the
    shard that owns their start row, and more than one shard contributes."""
    c = rr.rerank_case(rr.SHARD_CASE)
    want = rr.rerank_want(rr.SHARD_CASE, top)
    for cuts in c["cuts"]:
        merged, parts = rr.sharded_rerank_ref(c["index"], c["q"], c["ids"], c["item_row"], c["item_len"], top, cuts,
                                              c["max_len"], lattice=True)
        _same(merged, want, cuts)
        owners = sum(bool((p[0] >= 0).any()) for p in parts)
        assert owners == len(cuts) - 1
        assert min(hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])) < c["max_len"] - 1 or len(cuts) == 4
    # the planted run of the first item of every group is the best answer, whichever side of a cut it starts on
    first = c["item_row"][::3] // c["max_len"]
    assert len(set(first.tolist())) == len(first) and (want[0][::3, 0] >= 0).all()


@pytest.mark.parametrize("name", rr.MERGE_CASES)
def test_merge_c_restatement_over_the_case_table(name):
    """oracle_merge_topk equals merge_topk_ref bit for bit, and the case holds what its name says (rr.check_merge_case:
    ties, the entry moved to the last sweep is in the answer, holes, the special queries, the planted high ids)."""
    pd, pi, _ = rr.merge_case(name)
    ties = rr.check_merge_case(name)
    print(f"{name}: P*k = {pd.shape[0] * pd.shape[2]}, {ties} adjacent equal distances in the answer")
    _same(native.merge_topk(pd, pi)[::-1], rr.merge_want(name)[::-1], name)


def test_merge_reference_by_hand():
    """(distance, id) order, -1 skipped whatever its distance, +inf with a valid id before the padding."""
    inf = np.inf
    pd = np.array([[[0.5, 0.5, -3.0]], [[0.25, inf, 0.5]]], np.float32)
    pi = np.array([[[9, 2, -1]], [[4, 7, 1 << 33]]], np.int64)
    d, i = rr.merge_topk_ref(pd, pi)
    assert i.tolist() == [[4, 2, 9]] and d.tolist() == [[0.25, 0.5, 0.5]]
    wide_d, wide_i = np.full((1, 1, 6), inf, np.float32), np.full((1, 1, 6), -1, np.int64)
    wide_d[0, 0, :3], wide_i[0, 0, :3] = [inf, 1.0, inf], [7, 1 << 33, 3]
    d, i = rr.merge_topk_ref(wide_d, wide_i)
    assert i.tolist() == [[1 << 33, 3, 7, -1, -1, -1]] and d.tolist() == [[1.0, inf, inf, inf, inf, inf]]


def test_entry_points_refuse_before_any_launch():
    """grafp_seq_rerank_shard_f32 and grafp_row_sqnorm_f32 without a GPU: every call fails an argument check (or has no
    rows) before anything is launched; the pointers are never dereferenced.  top = 0 is refused as top, not as a null
    pointer (an output of zero columns has no storage), and an empty matrix needs no pointers at all."""
    import ctypes
    from grafp_amd._lib import lib
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(7)]

    def rerank(max_len=8, k=4, top=10, shard=(0, 100, 0, 100), rows=100, outs=(fake[5], fake[6])):
        row_base, n, id_lo, id_hi = shard
        rc = lib.grafp_seq_rerank_shard_f32(fake[0], rows, row_base, n, id_lo, id_hi, fake[1], 50, fake[2], k, fake[3],
                                            fake[4], 3, max_len, top, outs[0], outs[1], None)
        return rc, lib.grafp_last_error().decode()

    for kw, words in ((dict(max_len=63, k=33), "max_len=63 k=33 exceed"), (dict(max_len=65, k=1), "max_len=65 k=1 exceed"),
                      (dict(top=0, outs=(None, None)), "top=0 not in [1, 64]"), (dict(top=65), "top=65 not in [1, 64]"),
                      (dict(shard=(0, 100, 0, 51), rows=50), "bad shard rows"),
                      (dict(shard=(10, 100, 5, 20), rows=50), "bad shard rows"), (dict(outs=(None, fake[6])), "null pointer")):
        rc, msg = rerank(**kw)
        assert rc == -1 and msg.startswith("seq_rerank: ") and words in msg, (kw, msg)
    assert lib.grafp_row_sqnorm_f32(None, 0, 8, None, None) == 0
    assert lib.grafp_row_sqnorm_f32(None, 0, 153, None, None) == -1 and b"row_sqnorm: bad n=0 d=153" in lib.grafp_last_error()
    assert lib.grafp_row_sqnorm_f32(fake[0], 4, 153, fake[1], None) == -1 and b"d=153" in lib.grafp_last_error()
    assert lib.grafp_row_sqnorm_f32(None, 4, 8, fake[1], None) == -1 and b"row_sqnorm: null pointer" in lib.grafp_last_error()


def test_rerank_reference_by_hand():
    """Two candidates one period apart tie and come lowest id first; the start at n - 1 is scored over its one row."""
    index = np.zeros((6, rr.D), np.float32)
    index[[0, 3], 0], index[[1, 4], 0], index[5, 0] = 0.5, 0.25, -0.5
    q = np.zeros((2, rr.D), np.float32)
    q[0, 0], q[1, 0] = 0.5, 0.5
    ids = np.array([[3, 0, 5], [4, -1, 0]], np.int64)               # starts 3, 0, 5 | 3, -, -1 (dropped)
    i, s = rr.seq_rerank_ref(index, q, ids, [0], [2], 4, lattice=True)
    assert i.tolist() == [[0, 3, 5, -1]] and s.tolist() == [[0.1875, 0.1875, -0.25, -np.inf]]
    i, s = rr.seq_rerank_ref(index, q, ids, [0], [2], 2, max_len=1, lattice=True)
    assert i.tolist() == [[0, 3]] and s.tolist() == [[0.25, 0.25]]
    i, s = rr.seq_rerank_ref(index[2:], q, ids, [0], [2], 2, shard=(2, 6, 2, 4), lattice=True)
    assert i.tolist() == [[3, -1]]
