"""References and the case table of the sequence rerank (csrc/seq_rerank.hip) and the top-k merge (search_merge_kernel
in csrc/knn_search.hip).  TEST INFRASTRUCTURE; numpy only, nothing of oracle/ is imported here, so the GPU verdict of
tests/test_gpu_rerank.py does not rest on the C restatement (tests/test_rerank_cpu.py runs that one over the same table).

Two kinds of rerank input:
  * LATTICE: every element of index and q is j/8, j an integer in [-4, 4].  A product is an integer in units of 1/64
    (|.| <= 16), a span sum over at most 64 rows x 128 dims an integer below 2^17 in those units: exact in f32 in ANY
    summation order.  The reference sums in float64, asserts the sum equals its f32 rounding, and divides in f32
    (np.float32(sum) / np.float32(m)), so ids and score bits must equal the kernel's, equal scores included.  Ties are
    built on purpose: an index that repeats every PERIOD rows (cid and cid + PERIOD score alike) and all-zero query rows.
  * REAL (hash_normalish): the kernel's stated order is one fmaf chain of 4m terms per lane, five butterfly adds and one
    division, so |score - exact| <= (4m + 6) * 2^-24 * sum|q*x| / m =: bar (float64 sum).  Ids must match wherever the
    float64 scores of neighbouring entries of the ranking, the first dropped candidate included, differ by more than the
    sum of their two bars; inside a closer run the ids are compared as a set.  The share of output positions in such
    runs is computed from float64 alone (ambiguity) and must stay at or below 1 %.
"""
import functools

import numpy as np

from _hashfill import hash_ints, hash_normalish, hash_uniform

D = 128
EPS = 2.0 ** -24
PERIOD = 97
TOPS = (1, 10, 64)
I64_MAX = np.iinfo(np.int64).max


def lattice(name, shape):
    return hash_ints(name, shape, -4, 4).astype(np.float32) / np.float32(8.0)


# =============================================================== seq_rerank
def _spans(index, q, ids, item_row, item_len, max_len, shard):
    """Per item: (cid ascending unique, m, float64 span sum, float64 sum of |products|).  With a shard, `index` holds
    the global rows [row_base, row_base + len(index)) of an n-row index."""
    index64, q64 = np.asarray(index, dtype=np.float64), np.asarray(q, dtype=np.float64)
    ids = np.asarray(ids).astype(np.int64)
    row_base, n, id_lo, id_hi = (int(v) for v in shard) if shard is not None else (0, len(index64), 0, len(index64))
    assert ids.size == 0 or int(ids.max()) < n, "hit ids lie inside the index"
    out = []
    for r0, L in zip(np.asarray(item_row).astype(np.int64), np.asarray(item_len).astype(np.int64)):
        ql = int(L if max_len is None else min(L, max_len))
        t = np.arange(ql, dtype=np.int64)
        hit = ids[r0:r0 + ql]
        c = hit - t[:, None]                                              # a hit of segment t starts at id - t
        keep = (hit >= 0) & (c >= 0) & (c >= id_lo) & (c < id_hi)
        cid = np.unique(c[keep])
        m = np.minimum(ql, n - cid)
        assert (cid >= row_base).all() and (cid + m <= row_base + len(index64)).all(), "the sequence is not local"
        s, a = np.zeros(len(cid)), np.zeros(len(cid))
        step = max(1, 32768 // max(ql, 1))
        for b in range(0, len(cid), step):
            cc, mm = cid[b:b + step], m[b:b + step]
            live = t[None, :] < mm[:, None]
            rows = np.where(live, (cc - row_base)[:, None] + t[None, :], 0)
            prod = index64[rows] * q64[r0:r0 + ql][None]                  # (c, ql, D); f32 x f32 is exact in float64
            s[b:b + step] = (prod.sum(-1) * live).sum(-1)
            a[b:b + step] = (np.abs(prod).sum(-1) * live).sum(-1)
        out.append((cid, m, s, a))
    return out


def _pad_lists(n_items, top):
    return np.full((n_items, top), -1, np.int64), np.full((n_items, top), -np.inf, np.float32)


def seq_rerank_ref(index, q, ids, item_row, item_len, top, max_len=None, shard=None, lattice=False):
    """The definition in the header of seq_rerank.hip: (ids int64 (n_items, top), scores f32), best first by (score
    descending, id ascending), (-1, -inf) padded.  score = np.float32(float64 sum) / np.float32(m); lattice=True asserts
    that the sum IS an f32, which makes the score the one any f32 summation order gives."""
    out_i, out_s = _pad_lists(len(item_row), top)
    for it, (cid, m, s, _a) in enumerate(_spans(index, q, ids, item_row, item_len, max_len, shard)):
        s32 = s.astype(np.float32)
        if lattice:
            assert np.array_equal(s32.astype(np.float64), s), "a lattice span sum must be exact in f32"
        score = s32 / m.astype(np.float32)
        order = np.lexsort((cid, -score))[:top]
        out_i[it, :len(order)], out_s[it, :len(order)] = cid[order], score[order]
    return out_i, out_s


def merge_rerank_lists(part_i, part_s, top):
    """The rule of ShardedFlatL2Index.rerank over per-shard (n_items, top) lists: score descending, id ascending, empty
    slots last."""
    gi, gs = np.concatenate(part_i, axis=1), np.concatenate(part_s, axis=1)
    out_i, out_s = _pad_lists(gi.shape[0], top)
    for it in range(gi.shape[0]):
        order = np.lexsort((np.where(gi[it] < 0, I64_MAX, gi[it]), -gs[it]))[:top]
        out_i[it, :len(order)], out_s[it, :len(order)] = gi[it, order], gs[it, order]
    return out_i, out_s


def shard_calls(index, cuts, max_len):
    """[(rows, shard)] of an index cut at `cuts` (ascending, 0 first, n last): every shard gets its own rows and the
    next max_len - 1 of the index, so that every sequence starting in it is local."""
    n = len(index)
    return [(index[lo:min(n, hi + max_len - 1)], (lo, n, lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]


def sharded_rerank_ref(index, q, ids, item_row, item_len, top, cuts, max_len, lattice=False):
    """(merged (ids, scores), [per-shard (ids, scores)])."""
    parts = [seq_rerank_ref(rows, q, ids, item_row, item_len, top, max_len=max_len, shard=shard, lattice=lattice)
             for rows, shard in shard_calls(index, cuts, max_len)]
    return merge_rerank_lists([p[0] for p in parts], [p[1] for p in parts], top), parts


def tie_count(out_i, out_s):
    """Adjacent pairs of equal scores among the filled entries of the lists."""
    return int(((out_s[:, 1:] == out_s[:, :-1]) & (out_i[:, 1:] >= 0)).sum())


def _ranking(cid, m, s, a, top):
    """float64 ranking of one item, cut after the first dropped candidate: (ids, scores, bars, run label per entry)."""
    sc, bar = s / m, (4 * m + 6) * EPS * a / m
    order = np.lexsort((cid, -sc))[:top + 1]
    sc, bar = sc[order], bar[order]
    apart = (sc[:-1] - sc[1:]) > (bar[:-1] + bar[1:])
    return cid[order], sc, bar, np.concatenate([[0], np.cumsum(apart)]).astype(np.int64)


def ambiguity(index, q, ids, item_row, item_len, top, max_len=None, shard=None):
    """(output positions inside a run of scores closer than their bars, filled output positions): float64 alone."""
    amb = filled = 0
    for cid, m, s, a in _spans(index, q, ids, item_row, item_len, max_len, shard):
        _ids, _sc, _bar, run = _ranking(cid, m, s, a, top)
        nout = min(top, len(cid))
        amb += int((np.bincount(run)[run[:nout]] > 1).sum())
        filled += nout
    return amb, filled


def check_real(got_i, got_s, index, q, ids, item_row, item_len, top, max_len=None, shard=None):
    """Asserts a real-valued result against float64 (module docstring); returns (worst |score - exact| / bar, ambiguous
    positions, filled positions)."""
    worst, amb, filled = 0.0, 0, 0
    assert got_i.shape == (len(item_row), top) and got_s.shape == got_i.shape
    for it, (cid, m, s, a) in enumerate(_spans(index, q, ids, item_row, item_len, max_len, shard)):
        rid, _sc, _bar, run = _ranking(cid, m, s, a, top)
        nout = min(top, len(cid))
        gi, gs = got_i[it], got_s[it].astype(np.float64)
        assert (gi[nout:] == -1).all() and (got_s[it, nout:] == -np.inf).all(), ("padding", it)
        assert (gi[:nout] >= 0).all() and len(set(gi[:nout].tolist())) == nout, ("ids", it, gi)
        pos = np.searchsorted(cid, gi[:nout])
        assert (pos < len(cid)).all() and (cid[np.minimum(pos, len(cid) - 1)] == gi[:nout]).all(), ("not a candidate", it)
        dev, bar = np.abs(gs[:nout] - s[pos] / m[pos]), (4 * m[pos] + 6) * EPS * a[pos] / m[pos]
        assert (dev <= bar).all(), ("score beyond its bar", it, float((dev / np.maximum(bar, 1e-300)).max()))
        if nout:
            worst = max(worst, float((dev[bar > 0] / bar[bar > 0]).max(initial=0.0)))
        size = np.bincount(run)
        for j in range(nout):
            if size[run[j]] == 1:
                assert gi[j] == rid[j], ("id", it, j, int(gi[j]), int(rid[j]))
            else:
                assert gi[j] in set(rid[run == run[j]].tolist()), ("id outside its run", it, j, int(gi[j]))
        amb += int((size[run[:nout]] > 1).sum())
        filled += nout
    return worst, amb, filled


# ---- the rerank case table -------------------------------------------------------------------------------------------
def _items(nq, lens, n_items):
    rows, ln = [], []
    for i in range(n_items):
        L = lens[i % len(lens)]
        rows.append((i * 5) % (nq - L + 1))
        ln.append(L)
    return rows, ln


def _base(name, kind, n, nq, k, lens, n_items, q_off=11):
    """Index (periodic for lattice cases), query rows that follow index rows q_off + r (so an item at row r0 has the true
    start q_off + r0), hits: column 0 the true row, column 1 one period later, the rest anywhere in the index; k = 1
    alternates the two."""
    if kind == "lattice":
        index = np.tile(lattice(f"rr:{name}.index", (PERIOD, D)), (n // PERIOD + 1, 1))[:n].copy()
        q = index[(q_off + np.arange(nq)) % n].copy()
        q[:, :48] = lattice(f"rr:{name}.q", (nq, 48))
    else:
        # Rows that share one direction u with a strength of their own, plus noise: scores then spread over a range that
        # is wide against their bars (independent rows would give |score| ~ sum|q*x| / sqrt(128 m), and hundreds of
        # candidates a few bars apart: the ambiguous share is a property of the inputs, see ambiguity()).
        u = hash_normalish(f"rr:{name}.u", (1, D))
        index = (hash_uniform(f"rr:{name}.a", (n, 1)) * u + 0.25 * hash_normalish(f"rr:{name}.index", (n, D))).astype(np.float32)
        q = (index[(q_off + np.arange(nq)) % n] + 0.25 * hash_normalish(f"rr:{name}.q", (nq, D))).astype(np.float32)
    ids = hash_ints(f"rr:{name}.ids", (nq, k), 0, n - 1).astype(np.int64)
    if kind == "real":
        # as in retrieval, most hits of an item line up on a few diagonals (one start per column); one in ten is stray
        diag = (hash_ints(f"rr:{name}.diag", (1, k), 0, n - 1).astype(np.int64) + np.arange(nq)[:, None]) % n
        ids = np.where(hash_uniform(f"rr:{name}.stray", (nq, k)) < -0.8, ids, diag)
    true = (q_off + np.arange(nq)) % n
    later = np.where(true + PERIOD < n, true + PERIOD, true)
    if k == 1:
        ids[:, 0] = np.where(np.arange(nq) % 2 == 1, later, true)
    else:
        ids[:, 0], ids[:, 1] = true, later
    rows, ln = _items(nq, lens, n_items)
    return dict(name=name, kind=kind, index=index, q=q, ids=ids, rows=rows, lens=ln, k=k, max_len=None, ties=False,
                tops=TOPS, cuts=())


def _done(c):
    c["item_row"], c["item_len"] = np.asarray(c.pop("rows"), np.int64), np.asarray(c.pop("lens"), np.int32)
    c["n"], c["nq"] = len(c["index"]), len(c["q"])
    assert c["n"] <= 5000 and len(c["item_row"]) <= 600
    assert (c["item_row"] >= 0).all() and (c["item_row"] + c["item_len"] <= c["nq"]).all()
    assert int(c["item_len"].max(initial=0)) * c["k"] <= 2048 or c["max_len"] is not None
    return c


def _k32(kind):
    """k = 32 with 64, 1 and 33 segments: ql*k = 2048 (64 x 32), 32 and 1056; an all-zero query block (every score
    equal: lowest id first)."""
    c = _base(f"{kind}_k32", kind, 1000, 70, 32, (64, 1, 33), 12)
    if kind == "lattice":
        c["q"][66:70] = 0.0                                        # a silent query: every candidate scores +0
        c["rows"] += [66, 67]
        c["lens"] += [4, 1]
        c["ties"] = True
    return _done(c)


def _k2048(kind):
    """One segment, k = 2048 (ql*k = 2048 as 1 x 2048); the last item has 2048 distinct hits (second sort of 2048)."""
    c = _base(f"{kind}_k2048", kind, 3000, 5, 2048, (1,), 5)
    c["ids"][4] = (np.arange(2048, dtype=np.int64) * 7 + 3) % 3000        # 7 and 3000 are coprime: all distinct
    c["ties"] = kind == "lattice"
    return _done(c)


def _k1(kind):
    """k = 1: ql*k = 1, 63 and 64 (64 x 1); top 10 and 64 exceed the candidates of the short items (padding)."""
    c = _base(f"{kind}_k1", kind, 500, 70, 1, (64, 1, 63), 9)
    c["ties"] = kind == "lattice"
    return _done(c)


def _k6(kind):
    """k = 6, 3/5/1/19 segments, with -1 holes, hits smaller than their segment number, candidates that start at
    n-1 ... n-6 (m = 1 ... 6 rows, below ql), and an item of zero segments among the ordinary ones."""
    c = _base(f"{kind}_k6", kind, 300, 40, 6, (3, 5, 1, 19), 24)
    ids, n = c["ids"], 300
    ids[1, 3] = -1
    ids[7, :] = -1
    ids[9, 2:] = np.arange(4)                                       # item rows 5..: segment t >= 4 hits of id < t
    ids[15, :] = n - 1 - np.arange(6)                               # item 3 starts at row 15 with 19 segments: m = 1..6
    ids[16, :3] = n - 1                                             # start n - 2 through segment 1
    ids[20, :] = n - 1 - np.arange(6)                               # item 4 (rows 20..22): m = 1..3
    c["rows"] += [5, 0]
    c["lens"] += [0, 0]
    c["ties"] = kind == "lattice"
    return _done(c)


def _k41(kind):
    """ql*k = 1025 (25 x 41): one over 1024, the first sort runs at 2048 keys."""
    c = _base(f"{kind}_k41", kind, 2000, 30, 41, (25,), 4)
    c["ties"] = kind == "lattice"
    return _done(c)


def _k5():
    """ql*k = 65 (13 x 5) and 60, 5: just over the 64-key sort."""
    c = _base("lattice_k5", "lattice", 400, 20, 5, (13, 12, 1), 6)
    c["ties"] = True
    return _done(c)


def _unique():
    """Unique-candidate counts at k = 32, four segments each unless said: 0 (all -1), 0 (every hit smaller than its
    segment number), 1 (128 duplicates), exactly 64, exactly 65 (where the second sort's size goes from 64 to 128 while
    the first stays 128), 2048 distinct (64 segments) and 1024 distinct (32 segments: ql*k = 1024)."""
    c = _base("lattice_unique", "lattice", 3000, 84, 32, (1,), 0)
    ids = c["ids"]
    t4, j = np.arange(4)[:, None], np.arange(32)[None, :]
    ids[0:4] = -1
    ids[4:8] = np.minimum(hash_ints("rr:unique.small", (4, 32), 0, 3), t4 - 1)          # id < t; t = 0: -1
    ids[8:12] = 500 + t4
    ids[12:16] = 700 + t4 + (j + 32 * t4) % 64                                           # starts 700 .. 763
    ids[16:20] = ids[12:16]
    ids[19, 31] = 764 + 3                                                                # and 764
    t64 = np.arange(64)[:, None]
    ids[20:84] = t64 + 32 * t64 + j                                                      # starts 0 .. 2047
    c["rows"], c["lens"] = [0, 4, 8, 12, 16, 20, 20], [4, 4, 4, 4, 4, 64, 32]
    c["ties"], c["unique"] = True, [0, 0, 1, 64, 65, 2048, 1024]
    return _done(c)


def _negative():
    """Negative and mixed-sign scores: the query rows are the NEGATED index rows, so the true start scores most negative
    and the far hits around zero; item 0 has only the true start and its period twins (every score negative, tied)."""
    c = _base("lattice_negative", "lattice", 600, 40, 6, (7, 3, 12), 12)
    c["q"] = -c["index"][(11 + np.arange(40)) % 600]
    t = np.arange(7)
    c["ids"][0:7] = (11 + t)[:, None] + PERIOD * np.arange(6)[None, :]
    c["ties"] = True
    return _done(c)


def _clamp():
    """item_len above max_len: the kernel and the reference both use min(item_len, max_len) = 8 segments."""
    c = _base("lattice_clamp", "lattice", 600, 40, 6, (12, 3, 9, 8), 12)
    c["max_len"], c["ties"] = 8, True
    return _done(c)


def _many():
    """600 items that overlap in query rows (one workgroup each)."""
    c = _base("lattice_600items", "lattice", 1000, 200, 6, (3, 5, 1, 7), 600)
    c["ties"], c["tops"] = True, (10,)
    return _done(c)


def _shards():
    """An index cut into 3 shards, and into 5 of which one has 10 rows (fewer than max_len - 1 = 32): a true run is
    planted across every boundary and across the end of the index (hits only while the row exists)."""
    n, L = 1000, 33
    cuts3, cuts5 = (0, 334, 668, 1000), (0, 300, 310, 600, 900, 1000)
    starts = sorted({b - L // 2 for b in cuts3[1:] + cuts5[1:]} | {b - 1 for b in cuts5[1:-1]} | {n - 1, n - 5, 3})
    nq = len(starts) * L
    c = _base("lattice_shards", "lattice", n, nq, 8, (1,), 0)
    rows, lens = [], []
    for i, s in enumerate(starts):
        r = np.arange(L)
        src = np.minimum(s + r, n - 1)
        c["q"][i * L:(i + 1) * L, 48:] = c["index"][src, 48:]
        true = np.where(s + r < n, s + r, -1)
        c["ids"][i * L:(i + 1) * L, 0] = true
        c["ids"][i * L:(i + 1) * L, 1] = np.where((true >= 0) & (true + PERIOD < n), true + PERIOD, true)
        rows += [i * L, i * L + 2, i * L + 7]
        lens += [L, 5, 17]
    c["rows"], c["lens"], c["max_len"], c["ties"], c["cuts"], c["tops"] = rows, lens, L, True, (cuts3, cuts5), (1, 10)
    return _done(c)


_RERANK = {
    "lattice_k32": lambda: _k32("lattice"), "lattice_k2048": lambda: _k2048("lattice"), "lattice_k1": lambda: _k1("lattice"),
    "lattice_k6": lambda: _k6("lattice"), "lattice_k41": lambda: _k41("lattice"), "lattice_k5": _k5,
    "lattice_unique": _unique, "lattice_negative": _negative, "lattice_clamp": _clamp, "lattice_600items": _many,
    "lattice_shards": _shards,
    "real_k32": lambda: _k32("real"), "real_k2048": lambda: _k2048("real"), "real_k1": lambda: _k1("real"),
    "real_k6": lambda: _k6("real"), "real_k41": lambda: _k41("real"),
}
RERANK_CASES = tuple(_RERANK)
SHARD_CASE = "lattice_shards"


@functools.lru_cache(maxsize=None)
def rerank_case(name):
    """The inputs of one case, built once per process; callers must not modify the arrays."""
    c = _RERANK[name]()
    for a in (c["index"], c["q"], c["ids"], c["item_row"], c["item_len"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def rerank_want(name, top):
    """(ids, scores) of seq_rerank_ref for a case, computed once and shared by the tests."""
    c = rerank_case(name)
    out = seq_rerank_ref(c["index"], c["q"], c["ids"], c["item_row"], c["item_len"], top, max_len=c["max_len"],
                         lattice=c["kind"] == "lattice")
    for a in out:
        a.setflags(write=False)
    return out


# =============================================================== merge_topk
def merge_topk_ref(part_d, part_i):
    """(P, nq, k) partial lists -> (nq, k): the entries with id >= 0 ordered by (distance, id), the first k, padded with
    (+inf, -1).  Selection only: the output distances are input bits."""
    part_d, part_i = np.asarray(part_d, np.float32), np.asarray(part_i).astype(np.int64)
    P, nq, k = part_d.shape
    d, i = part_d.transpose(1, 0, 2).reshape(nq, P * k), part_i.transpose(1, 0, 2).reshape(nq, P * k)
    out_d, out_i = np.full((nq, k), np.inf, np.float32), np.full((nq, k), -1, np.int64)
    for qi in range(nq):
        v = np.flatnonzero(i[qi] >= 0)
        o = v[np.lexsort((i[qi, v], d[qi, v]))[:k]]
        out_d[qi, :len(o)], out_i[qi, :len(o)] = d[qi, o], i[qi, o]
    return out_d, out_i


HI_BASE = 1 << 33
# planted in query 0 of the high-id cases, all at one distance below every other: expected in this order
HI_PLANT = (HI_BASE + 5, HI_BASE + 7, HI_BASE + (1 << 31) + 6, HI_BASE + (1 << 32) + 5)

# name: (P, k, nq, distances, order of the entries along the sweep, share of -1 holes, special queries, ids above 2^32)
_MERGE = {
    "pk20_k20": (1, 20, 37, "grid", "hash", 0.0, True, False),
    "pk2048_k32_holes": (64, 32, 37, "grid", "hash", 0.3, True, False),
    "pk2049_k1": (2049, 1, 37, "grid", "hash", 0.0, False, False),
    "pk2049_k1_tie_in_last_sweep": (2049, 1, 37, "grid", "tie_last", 0.0, False, False),
    "pk6176_k32_best_first": (193, 32, 37, "grid", "best_first", 0.0, False, False),
    "pk6176_k32_best_last": (193, 32, 37, "grid", "best_last", 0.0, False, False),
    "pk6176_k32_tie_in_last_sweep": (193, 32, 37, "grid", "tie_last", 0.0, False, False),
    "pk6176_k32_distinct_best_last_nq1": (193, 32, 1, "distinct", "best_last", 0.0, False, False),
    "pk6200_k20_holes_high_ids": (310, 20, 37, "grid", "hash", 0.3, True, True),
    "pk6176_k32_high_ids_best_last_nq1": (193, 32, 1, "grid", "best_last", 0.0, False, True),
    "pk6200_k20_tie_in_last_sweep_high_ids": (310, 20, 37, "grid", "tie_last", 0.0, False, True),
}
MERGE_CASES = tuple(_MERGE)


@functools.lru_cache(maxsize=None)
def merge_case(name):
    """(part_d (P, nq, k) f32, part_i (P, nq, k) int64, info).  Entry e = p*k + j of a query is read in sweep e // 2048.
    Special queries (nq = 37): 1 all -1; 2 fewer than k valid entries; 3 fewer than k valid, two of them at +inf."""
    P, k, nq, dist, order, holes, special, high = _MERGE[name]
    total = P * k
    if dist == "grid":
        d = hash_ints(f"mg:{name}.d", (nq, total), 0, 15).astype(np.float32) / np.float32(4.0)
    else:
        d = np.argsort(np.argsort(hash_uniform(f"mg:{name}.d", (nq, total)), axis=1), axis=1).astype(np.float32) * 0.5
    v = np.argsort(hash_uniform(f"mg:{name}.i", (nq, total)), axis=1).astype(np.int64)      # a permutation per query
    if high:   # words of the id: high = 2 + v % 4, bit 31 of the low word = (v / 4) % 2, the rest of the low word
        ids = HI_BASE + ((v % 4) << 32) + (((v // 4) % 2) << 31) + v // 8 + 100
    else:
        ids = v * 3 + 1
    info, at = {}, []
    if order != "hash":
        for qi in range(nq):
            o = np.lexsort((ids[qi], d[qi]))
            o = o if order != "best_last" else o[::-1]
            d[qi], ids[qi] = d[qi, o], ids[qi, o]
        if order == "tie_last":     # ascending; the lowest id at the k-th distance goes to the very end
            assert total > 2048 and (d[:, k] == d[:, k - 1]).all(), "a tie at the k-th distance"
            first = np.array([np.flatnonzero(d[qi] == d[qi, k - 1])[0] for qi in range(nq)])
            for qi in range(nq):
                f = first[qi]
                d[qi, [f, total - 1]], ids[qi, [f, total - 1]] = d[qi, [total - 1, f]], ids[qi, [total - 1, f]]
            info["moved"] = ids[:, total - 1].copy()
    if high and order == "hash":
        at = [5 % total, total // 3, (2 * total) // 3, total - 1]
        d[0, at], ids[0, at] = -1.0, HI_PLANT[::-1]
    if holes:
        hole = hash_uniform(f"mg:{name}.hole", (nq, total)) < (2.0 * holes - 1.0)
        hole[0, at] = False
        if special:
            hole[1:4] = False
        ids[hole] = -1
        d[hole & (hash_uniform(f"mg:{name}.hd", (nq, total)) < 0.0)] = -2.0          # a hole that looks best of all
    if special:
        ids[1] = -1
        keep = np.argsort(hash_uniform(f"mg:{name}.keep", (2, total)), axis=1)[:, :max(1, k - 3)]
        for row, kp in ((2, keep[0]), (3, keep[1])):
            gone = np.ones(total, bool)
            gone[kp] = False
            ids[row, gone] = -1
        d[3, keep[1][:2]] = np.inf
    part = lambda a: np.ascontiguousarray(a.reshape(nq, P, k).transpose(1, 0, 2))
    pd, pi = part(d), part(ids)
    pd.setflags(write=False)
    pi.setflags(write=False)
    return pd, pi, info


@functools.lru_cache(maxsize=None)
def merge_want(name):
    pd, pi, _ = merge_case(name)
    out = merge_topk_ref(pd, pi)
    for a in out:
        a.setflags(write=False)
    return out


def check_merge_case(name):
    """What a case promises about its own inputs and answer (asserted by the CPU test): returns the tie count."""
    P, k, nq, dist, order, holes, special, high = _MERGE[name]
    pd, pi, info = merge_case(name)
    wd, wi = merge_want(name)
    ties = int(((wd[:, 1:] == wd[:, :-1]) & (wi[:, 1:] >= 0)).sum())
    if dist == "distinct":
        assert ties == 0
    elif k > 1:
        assert ties > 0
    if order == "tie_last":           # the entry moved to the last sweep belongs into the answer
        assert all(info["moved"][qi] in wi[qi] for qi in range(nq))
    if holes:
        share = float((pi < 0).mean())
        assert 0.25 < share < 0.4 and (wi[0] >= 0).all()
        assert (pd[pi < 0] == -2.0).any() and (wd > -2.0).all()              # no hole's distance came through
    if special:
        assert (wi[1] == -1).all() and (wd[1] == np.inf).all()
        nv = max(1, k - 3)
        for row in (2, 3):
            assert (wi[row, :nv] >= 0).all() and (wi[row, nv:] == -1).all() and (wd[row, nv:] == np.inf).all()
        if nv >= 3:
            assert (wd[3, nv - 2:nv] == np.inf).all() and (wi[3, nv - 2:nv] >= 0).all() and np.isfinite(wd[3, nv - 3])
    if high:
        assert int(wi[wi >= 0].min()) >= HI_BASE
        if order == "hash":
            assert tuple(wi[0, :4]) == HI_PLANT
    return ties


# =============================================================== row_sqnorm
def row_sqnorm_ref(x):
    """float64 (sum of squares, the same: every term is non-negative) per row."""
    x = np.asarray(x, np.float64)
    return (x * x).sum(axis=1)
