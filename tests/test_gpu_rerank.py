"""The sequence rerank (seq_rerank_kernel, csrc/seq_rerank.hip) and the top-k merge (search_merge_kernel, csrc/knn_search.hip)
on the MI355X against the numpy references and the case table of tests/_rerank_ref.py -- lattice inputs and every merge case
bit for bit (ids and float bits, ties included), real-valued inputs within the bar that follows from the kernel's stated
summation order -- plus ops.row_sqnorm at its edge sizes and ops.search_l2 split over several launches.  The C restatement
(oracle/) takes no part in these verdicts; tests/test_rerank_cpu.py runs it over the same table."""
import numpy as np
import pytest
import torch

import _rerank_ref as rr
from _hashfill import hash_normalish
from grafp_amd import ops
from grafp_amd._lib import lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.array(a))                   # a copy: the shared case arrays are read-only


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got = [g.cpu().numpy() if torch.is_tensor(g) else g for g in got]
    assert got[0].shape == want[0].shape and got[0].dtype == want[0].dtype and got[1].dtype == want[1].dtype, what
    assert np.array_equal(got[0], want[0]), (what, "ids", np.argwhere(got[0] != want[0])[:5])
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, "floats", np.argwhere(_bits(got[1]) != _bits(want[1]))[:5])


def _given_len(c):
    return int(c["max_len"] if c["max_len"] is not None else c["item_len"].max())


def _args(c, dev):
    return [t(c[key]).to(dev) for key in ("index", "q", "ids", "item_row", "item_len")]


def _rerank(c, dev, top, **kw):
    kw.setdefault("max_len", _given_len(c))
    got = ops.seq_rerank(*_args(c, dev), top=top, **kw)
    return got[0].cpu().numpy(), got[1].cpu().numpy()


# =============================================================== seq_rerank
@pytest.mark.parametrize("name", rr.RERANK_CASES)
def test_seq_rerank_case_table(dev, name):
    """ops.seq_rerank over the table of tests/_rerank_ref.py at top 1, 10 and 64 (above and below the candidate count).
    lattice_*: ids and score bits equal the float64-exact reference (any f32 summation order gives these bits), equal
    scores lowest id first -- k32: ql*k = 2048 as 64 x 32 and a silent all-zero query; k2048: 1 x 2048 and 2048 unique
    candidates; k1: ql*k = 1, 63, 64 (64 x 1), padding; k5 / k41: 65 and 1025 keys; k6: -1 holes, hits below their segment
    number, starts at n-1 ... n-6 (m below ql, down to 1), an item of zero segments; unique: 0, 1, exactly 64 and 65
    (second sort 64 -> 128), 1024 and 2048 unique candidates; negative: negative and mixed-sign scores through the
    order-preserving integer key; clamp: item_len above max_len; 600items: 600 overlapping items.
    real_*: every score within (4m + 6) * 2^-24 * sum|q*x| / m of float64, ids equal outside runs closer than their bars."""
    c = rr.rerank_case(name)
    for top in c["tops"]:
        got = _rerank(c, dev, top)
        if c["kind"] == "lattice":
            want = rr.rerank_want(name, top)
            print(f"{name} top {top}: bit-exact case, ambiguous share 0, {rr.tie_count(*want)} tied neighbours")
            _same(got, want, (name, top))
        else:
            worst, amb, filled = rr.check_real(got[0], got[1], c["index"], c["q"], c["ids"], c["item_row"], c["item_len"],
                                               top, max_len=c["max_len"])
            print(f"{name} top {top}: worst score deviation {worst:.3f} of its bar, ambiguous share {amb}/{filled}, "
                  f"{rr.tie_count(*got)} tied neighbours")
            assert amb <= 0.01 * filled


@pytest.mark.parametrize("name", ["lattice_k6", "lattice_k32", "real_k6"])
def test_seq_rerank_checking_path_gives_the_same_bits(dev, name):
    """max_len=None (the wrapper finds the longest item and checks the items against q_rows) == max_len given, and a
    larger bound changes nothing either."""
    c = rr.rerank_case(name)
    given = _rerank(c, dev, 10)
    _same(_rerank(c, dev, 10, max_len=None), given, name)
    if _given_len(c) * c["k"] < 2048:
        _same(_rerank(c, dev, 10, max_len=min(64, 2048 // c["k"])), given, name)
    if c["kind"] == "lattice":
        _same(given, rr.rerank_want(name, 10), name)


def test_seq_rerank_input_types(dev):
    """float64 and non-contiguous index_rows / q_rows, int32 topk_ids and item_row, int64 item_len: the same bits as the
    contiguous f32 / int64 / int32 copies."""
    c = rr.rerank_case("lattice_k6")
    index, q, ids, item_row, item_len = _args(c, dev)
    want = rr.rerank_want("lattice_k6", 10)
    wide = torch.full((c["n"], 2 * rr.D), float("nan"), dtype=torch.float64, device=dev)
    wide[:, ::2] = index.double()
    qwide = torch.full((2 * c["nq"], rr.D), float("nan"), device=dev)
    qwide[::2] = q
    assert not wide[:, ::2].is_contiguous() and not qwide[::2].is_contiguous()
    _same(ops.seq_rerank(wide[:, ::2], qwide[::2], ids, item_row, item_len, top=10), want, "f64 / strided rows")
    _same(ops.seq_rerank(index, q.double(), ids.to(torch.int32), item_row.to(torch.int32), item_len.to(torch.int64),
                         top=10, max_len=19), want, "int32 ids")
    _same(ops.seq_rerank(index, q, ids.t().contiguous().t(), item_row, item_len, top=10), want, "strided ids")


def test_seq_rerank_no_items(dev):
    """n_items = 0: empty (0, top) outputs of the right types, on both call forms and with a shard."""
    c = rr.rerank_case("lattice_k6")
    index, q, ids, item_row, item_len = _args(c, dev)
    for kw in (dict(), dict(max_len=19), dict(max_len=19, shard=(0, c["n"], 0, c["n"]))):
        i, s = ops.seq_rerank(index, q, ids, item_row[:0], item_len[:0], top=7, **kw)
        assert i.shape == (0, 7) and s.shape == (0, 7) and i.dtype == torch.int64 and s.dtype == torch.float32


@pytest.mark.parametrize("which", [0, 1])
def test_seq_rerank_shards_in_one_process(dev, which):
    """The shard= form of ops.seq_rerank, every shard on this device: an index cut into 3, and into 5 where one shard has
    10 rows (fewer than max_len - 1 = 32, so its call reads on into the shards after it).  Every call gets
    rows[lo : min(n, hi + max_len - 1)] and shard=(lo, n, lo, hi); its list equals seq_rerank_ref(shard=...) bit for bit,
    and the lists merged by the rule of ShardedFlatL2Index.rerank equal the unsharded kernel and the unsharded reference.
    True runs are planted across every boundary and across the end of the index."""
    c = rr.rerank_case(rr.SHARD_CASE)
    cuts, L = c["cuts"][which], c["max_len"]
    _index, q, ids, item_row, item_len = _args(c, dev)
    for top in c["tops"]:
        (_mi, _ms), parts = rr.sharded_rerank_ref(c["index"], c["q"], c["ids"], c["item_row"], c["item_len"], top, cuts, L,
                                                  lattice=True)
        got = []
        for (rows, shard), want in zip(rr.shard_calls(c["index"], cuts, L), parts):
            g = ops.seq_rerank(t(rows).to(dev), q, ids, item_row, item_len, top=top, shard=shard, max_len=L)
            got.append((g[0].cpu().numpy(), g[1].cpu().numpy()))
            _same(got[-1], want, (cuts, top, shard))
        merged = rr.merge_rerank_lists([g[0] for g in got], [g[1] for g in got], top)
        _same(merged, rr.rerank_want(rr.SHARD_CASE, top), (cuts, top))
        _same(_rerank(c, dev, top), merged, (cuts, top, "one index"))
        print(f"cuts {cuts} top {top}: {len(parts)} shards bit-exact, {rr.tie_count(*merged)} tied neighbours")


def test_sharded_index_of_one_rank_reranks_through_the_shard_form(dev):
    """FlatL2Index + dist.ShardedFlatL2Index (world 1): search, then .rerank, which passes shard=(0, n, 0, n).  Lattice
    rows make the squared distances exact too: the search equals float64 by (distance, id) -- rows one period apart are
    equal, so ties abound -- and the rerank of the search's own hits equals the reference bit for bit."""
    from grafp_amd.dist import ShardedFlatL2Index
    c = rr.rerank_case("lattice_k6")
    index = ShardedFlatL2Index(rr.D)
    index.add_global(c["index"].copy())
    assert index.world == 1 and (index.lo, index.hi, index.ntotal) == (0, c["n"], c["n"])
    D, I = index.search(c["q"].copy(), c["k"])
    x, q = c["index"].astype(np.float64), c["q"].astype(np.float64)
    d64 = (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * q @ x.T
    order = np.stack([np.lexsort((np.arange(c["n"]), d64[r]))[:c["k"]] for r in range(c["nq"])])
    assert np.array_equal(I, order) and np.array_equal(D.astype(np.float64), np.take_along_axis(d64, order, 1))
    got = index.rerank(c["q"].copy(), I, c["item_row"].copy(), c["item_len"].copy(), top=10)
    want = rr.seq_rerank_ref(c["index"], c["q"], I, c["item_row"], c["item_len"], 10, lattice=True)
    print(f"world 1: {int((D[:, 1:] == D[:, :-1]).sum())} tied distances, {rr.tie_count(*want)} tied scores")
    _same(got, want, "world 1")


def test_seq_rerank_refusals(dev):
    """The kernel's own refusals name the operation and write nothing: max_len * k > 2048, max_len > 64, top of 0 and of
    65, a shard whose id_hi exceeds row_base + rows (all refused by the entry point before a launch: outputs handed to
    it directly keep their fill), and an item that reaches outside q_rows on the max_len=None path.  top = 0 used to be
    reported as 'null pointer' (the wrapper's (n_items, 0) outputs have no storage and the pointers were tested first);
    the entry point now tests top before them."""
    c = rr.rerank_case("lattice_k32")
    index, q, ids, item_row, item_len = _args(c, dev)
    n, nq, n_items = c["n"], c["nq"], len(c["item_row"])
    ids33 = torch.cat([ids, ids[:, :1]], dim=1).contiguous()

    def entry(ids_, max_len, top, shard=None, rows=index):
        row_base, n_total, id_lo, id_hi = shard or (0, n, 0, n)
        out_i = torch.full((n_items, max(top, 1)), -7, dtype=torch.int64, device=dev)
        out_s = torch.full((n_items, max(top, 1)), 123.0, device=dev)
        p = ops._p
        rc = lib.grafp_seq_rerank_shard_f32(p(rows), rows.shape[0], row_base, n_total, id_lo, id_hi, p(q), nq, p(ids_),
                                            ids_.shape[1], p(item_row), p(item_len), n_items, max_len, top, p(out_i),
                                            p(out_s), ops._stream())
        torch.cuda.synchronize()
        assert rc != 0 and (out_i == -7).all() and (out_s == 123.0).all()
        assert "seq_rerank" in lib.grafp_last_error().decode()

    entry(ids33, 63, 10)                                             # 63 * 33 = 2079 candidates
    entry(ids[:, :1].contiguous(), 65, 10)
    entry(ids, 64, 0)
    entry(ids, 64, 65)
    entry(ids, 64, 10, shard=(0, n, 0, 501), rows=index[:500])
    with pytest.raises(RuntimeError, match="seq_rerank.*max_len=63 k=33"):
        ops.seq_rerank(index, q, ids33, item_row, item_len, top=10, max_len=63)
    with pytest.raises(RuntimeError, match="seq_rerank.*max_len=65"):
        ops.seq_rerank(index, q, ids[:, :1], item_row, item_len, top=10, max_len=65)
    for top in (0, 65):
        with pytest.raises(RuntimeError, match=f"seq_rerank: top={top}"):
            ops.seq_rerank(index, q, ids, item_row, item_len, top=top, max_len=64)
    with pytest.raises(RuntimeError, match="seq_rerank: bad shard"):
        ops.seq_rerank(index[:500], q, ids, item_row, item_len, top=10, max_len=64, shard=(0, n, 0, 501))
    outside = item_row.clone()
    outside[1] = nq                                                  # one segment, one row past the end
    with pytest.raises(ValueError, match="seq_rerank: an item reaches outside q_rows"):
        ops.seq_rerank(index, q, ids, outside, item_len, top=10)
    outside[1] = -1
    with pytest.raises(ValueError, match="seq_rerank: an item reaches outside q_rows"):
        ops.seq_rerank(index, q, ids, outside, item_len, top=10)


# =============================================================== merge_topk
@pytest.mark.parametrize("name", rr.MERGE_CASES)
def test_merge_topk_case_table(dev, name):
    """ops.merge_topk == merge_topk_ref, ids and distance bits.  P*k of 20, 2048 (one full sweep), 2049 (a second sweep of
    one entry) and 6176 / 6200 (three sweeps and a remainder; later sweeps are pruned by the running threshold); k of 1,
    20, 32; nq of 1 and 37; distances on a grid of 16 values (ties everywhere) or all distinct.  best_last: the final sweep
    replaces the whole list; best_first: everything after the first sweep may be pruned; tie_in_last_sweep: the lowest id
    at the k-th distance arrives last and must still get in (the threshold test must admit equality); holes: 30 % of the
    entries are -1, half of them with a distance below every valid one; special queries: all -1, fewer than k valid, a
    valid id at +inf (sorts before the padding, keeps its id); high_ids: ids above 2^33 whose order is decided by the
    high word only, by the low word only, and by bit 31 of the low word."""
    pd, pi, _ = rr.merge_case(name)
    want = rr.merge_want(name)
    got = ops.merge_topk(t(pd).to(dev), t(pi).to(dev))
    ties = int(((want[0][:, 1:] == want[0][:, :-1]) & (want[1][:, 1:] >= 0)).sum())
    print(f"{name}: P*k = {pd.shape[0] * pd.shape[2]}, nq = {pd.shape[1]}, {ties} tied neighbours, bit-exact case")
    _same(got[::-1], want[::-1], name)


def test_merge_topk_input_types(dev):
    """int32 part_i, float64 part_d and non-contiguous lists: the same bits as their converted copies."""
    name = "pk2048_k32_holes"
    pd, pi, _ = rr.merge_case(name)
    want = rr.merge_want(name)
    got = ops.merge_topk(t(pd).to(dev).double(), t(pi).to(dev).to(torch.int32))
    _same(got[::-1], want[::-1], "int32 ids")
    swapped_d, swapped_i = t(pd.transpose(1, 0, 2)).to(dev), t(pi.transpose(1, 0, 2)).to(dev)
    got = ops.merge_topk(swapped_d.transpose(0, 1), swapped_i.transpose(0, 1))
    _same(got[::-1], want[::-1], "strided lists")


# =============================================================== row_sqnorm
@pytest.mark.parametrize("d", [1, 3, 128, 152])
def test_row_sqnorm_small_shapes(dev, d):
    """d of 1, 3, 128 and 152 (the largest the kernel's tile takes) at n of 1, 255, 256 and 257 (one row, one short of a
    256-row tile, the tile, a second workgroup of one row).  Lattice rows (j/8): sums of at most 152 squares are integers
    in units of 1/64, exact in f32, compared exactly with float64.  Real rows: one fmaf chain of d terms, so within
    (d + 1) * 2^-24 * sum x^2 of float64."""
    worst = 0.0
    for n in (1, 255, 256, 257):
        x = rr.lattice(f"sq:{n}.{d}", (n, d))
        got = ops.row_sqnorm(t(x).to(dev))
        assert got.shape == (n,) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().astype(np.float64), rr.row_sqnorm_ref(x)), (n, d)
        x = hash_normalish(f"sq:real.{n}.{d}", (n, d))
        want = rr.row_sqnorm_ref(x)
        dev_ = np.abs(ops.row_sqnorm(t(x).to(dev)).cpu().numpy().astype(np.float64) - want)
        bar = (d + 1) * rr.EPS * want
        assert (dev_ <= bar).all(), (n, d, float((dev_ / bar).max()))
        worst = max(worst, float((dev_[bar > 0] / bar[bar > 0]).max(initial=0.0)))
    print(f"row_sqnorm d={d}: lattice rows exact, real rows at most {worst:.3f} of the bar")


def test_row_sqnorm_second_grid_stride_trip(dev):
    """n = 2048 * 256 + 300 rows at d = 8 (16 MB): the launch is capped at 2048 workgroups, so the first two start a second
    trip, the second of them on a partial tile.  Lattice rows, exact."""
    n, d = 2048 * 256 + 300, 8
    x = rr.lattice("sq:stride", (n, d))
    got = ops.row_sqnorm(t(x).to(dev)).cpu().numpy()
    want = rr.row_sqnorm_ref(x)
    bad = np.flatnonzero(got.astype(np.float64) != want)
    print(f"row_sqnorm n={n} d={d}: {len(bad)} rows differ")
    assert len(bad) == 0, bad[:5]


def test_row_sqnorm_refusal_and_empty(dev):
    """d = 153 is refused by name; n = 0 gives an empty tensor (an empty matrix has no storage: the entry point must not
    ask for its pointers; it did, and row_sqnorm of a (0, d) tensor failed with 'null pointer' until it returned first)."""
    with pytest.raises(RuntimeError, match="row_sqnorm.*d=153"):
        ops.row_sqnorm(torch.zeros((4, 153), device=dev))
    for d in (8, 128):
        out = ops.row_sqnorm(torch.empty((0, d), device=dev))
        assert out.shape == (0,) and out.dtype == torch.float32 and out.device.type == "cuda"
    with pytest.raises(RuntimeError, match="row_sqnorm.*d=153"):
        ops.row_sqnorm(torch.empty((0, 153), device=dev))


# =============================================================== search_l2
def test_search_l2_split_over_launches(dev):
    """max_queries_per_launch = 7 on 20 queries (launches of 7, 7 and 6) against a 3000-row database: both paths, f32 and
    bf16 pre-filter, give the bits of one launch."""
    db = hash_normalish("gpu:split.db", (3000, 128))
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    q = (db[(np.arange(20) * 131) % 3000] + 0.05 * hash_normalish("gpu:split.q", (20, 128))).astype(np.float32)
    dbt, qt = t(db).to(dev), t(q).to(dev)
    sq, bf = ops.row_sqnorm(dbt), ops.rows_to_bf16(dbt)
    for kw in (dict(), dict(db_bf16=bf)):
        one = ops.search_l2(dbt, sq, qt, 10, id_base=5, **kw)
        split = ops.search_l2(dbt, sq, qt, 10, id_base=5, max_queries_per_launch=7, **kw)
        assert torch.equal(one[1], split[1]) and torch.equal(one[0].view(torch.int32), split[0].view(torch.int32))
        assert torch.equal(one[1][:, 0].cpu(), t((np.arange(20) * 131) % 3000 + 5))
    print("search_l2: 3 launches of <= 7 queries equal one launch on both paths")


def test_flat_index_search_on_an_empty_index(dev):
    """FlatL2Index.search before any add: (+inf, -1) of the asked shape, numpy in -> numpy out and tensors alike."""
    index = ops.FlatL2Index(128, device=dev)
    D, I = index.search(np.zeros((3, 128), np.float32), 4)
    assert D.shape == (3, 4) and D.dtype == np.float32 and (D == np.inf).all() and I.dtype == np.int64 and (I == -1).all()
    D, I = index.search(torch.zeros((2, 128), device=dev), 1)
    assert D.shape == (2, 1) and bool((D == float("inf")).all()) and bool((I == -1).all()) and I.dtype == torch.int64
