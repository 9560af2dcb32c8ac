"""numpy restatement of grafp_cross_match_f32 (csrc/crossmatch.hip, include/grafp_hip.h): the contract the kernels are
tested against.  Scores use _identify_ref.score_runs, the arithmetic order of grafp_identify_f32 (one fmaf chain per
lane, butterfly 16-8-4-2-1, one f32 division).  grafp_cross_match_pq_f32 is cross_match_pq_ref: the same restatement on
_identify_pq_ref.decode(...)."""
import numpy as np

from _identify_pq_ref import decode
from _identify_ref import score_runs


def eligible_candidates(n, first, ids, min_votes=4, min_overlap=1):
    """One source, ids (L, k) the hits of its rows -> its eligible candidates [(b, delta, votes, i_lo, m)], in no
    particular order.  Nothing is dropped but ids outside [0, n)."""
    first = np.asarray(first, np.int64)
    ids = np.asarray(ids, np.int64)
    T = first.shape[0] - 1
    cand = {}                                       # (b, delta) -> [votes, i_lo, i_hi]
    for i in range(ids.shape[0]):
        for r in ids[i].tolist():
            if not 0 <= r < n:
                continue
            b = min(int(np.searchsorted(first, r, side="right")) - 1, T - 1)
            key = (b, r - int(first[b]) - i)
            c = cand.get(key)
            if c is None:
                cand[key] = [1, i, i]
            else:
                c[0] += 1
                c[1], c[2] = min(c[1], i), max(c[2], i)
    return [(b, d, v, lo, hi - lo + 1) for (b, d), (v, lo, hi) in cand.items()
            if v >= min_votes and hi - lo + 1 >= min_overlap]


def cross_match_source(index_rows, first, q, ids, top=8, min_votes=4, min_overlap=1):
    """One source: q (L, 128) its rows, ids (L, k) their library hits -> list of (b, delta, i_lo, m, score, votes), best
    first."""
    index_rows = np.asarray(index_rows, np.float32)
    first = np.asarray(first, np.int64)
    elig = eligible_candidates(index_rows.shape[0], first, ids, min_votes, min_overlap)
    best = {}
    if elig:
        e = np.array(elig, np.int64)
        scores = score_runs(q, index_rows, e[:, 3], first[e[:, 0]] + e[:, 1] + e[:, 3], e[:, 4])
        for (b, d, v, lo, m), sc in zip(elig, scores):
            cur = best.get(b)
            if cur is None or sc > cur[3] or (sc == cur[3] and d < cur[0]):
                best[b] = (d, lo, m, sc, v)
    ranked = sorted(best.items(), key=lambda kv: (-kv[1][3], kv[0]))[:top]
    return [(b, d, lo, m, sc, v) for b, (d, lo, m, sc, v) in ranked]


def cross_match_ref(index_rows, first, q_rows, src_first, ids, top=8, min_votes=4, min_overlap=1):
    """All sources -> (b, delta, i_lo, m, score, votes) arrays (S, top), padded like the kernel with
    -1 / INT_MIN / -1 / 0 / -inf / 0."""
    q_rows, ids = np.asarray(q_rows, np.float32), np.asarray(ids, np.int64)
    src_first = np.asarray(src_first, np.int64)
    ns = len(src_first) - 1
    b_ = np.full((ns, top), -1, np.int32)
    d_ = np.full((ns, top), np.iinfo(np.int32).min, np.int32)
    lo_ = np.full((ns, top), -1, np.int32)
    m_ = np.zeros((ns, top), np.int32)
    sc_ = np.full((ns, top), -np.inf, np.float32)
    v_ = np.zeros((ns, top), np.int32)
    for s in range(ns):
        r0, r1 = int(src_first[s]), int(src_first[s + 1])
        for j, (b, d, lo, m, sc, v) in enumerate(cross_match_source(index_rows, first, q_rows[r0:r1], ids[r0:r1], top,
                                                                    min_votes, min_overlap)):
            b_[s, j], d_[s, j], lo_[s, j], m_[s, j], sc_[s, j], v_[s, j] = b, d, lo, m, sc, v
    return b_, d_, lo_, m_, sc_, v_


def cross_match_pq_ref(list_id, codes, centroids, codebooks, first, q_rows, src_first, ids, top=8, min_votes=4,
                       min_overlap=1):
    return cross_match_ref(decode(list_id, codes, centroids, codebooks), first, q_rows, src_first, ids, top, min_votes,
                           min_overlap)
