"""numpy restatement of grafp_self_match_f32 (csrc/selfmatch.hip, include/grafp_hip.h): the contract the kernel is tested
against.  Scores use _identify_ref.score_runs, the arithmetic order of grafp_identify_f32 (one fmaf chain per lane,
butterfly 16-8-4-2-1, one f32 division)."""
import numpy as np

from _identify_ref import score_runs


def eligible_candidates(index_rows, first, ids, a, min_votes=4, min_overlap=1):
    """Source track a -> its eligible candidates [(b, delta, votes, i_lo, m)], in no particular order."""
    first = np.asarray(first, np.int64)
    ids = np.asarray(ids, np.int64)
    n, T = int(np.asarray(index_rows).shape[0]), first.shape[0] - 1
    fa, fb = int(first[a]), int(first[a + 1])
    cand = {}                                       # (b, delta) -> [votes, i_lo, i_hi]
    for i in range(fb - fa):
        for r in ids[fa + i].tolist():
            if not 0 <= r < n or fa <= r < fb:
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


def self_match_track(index_rows, first, ids, a, top=8, min_votes=4, min_overlap=1):
    """Source track a -> list of (b, delta, i_lo, m, score, votes), best first."""
    index_rows = np.asarray(index_rows, np.float32)
    first = np.asarray(first, np.int64)
    fa = int(first[a])
    elig = eligible_candidates(index_rows, first, ids, a, min_votes, min_overlap)
    best = {}
    if elig:
        e = np.array(elig, np.int64)
        scores = score_runs(index_rows, index_rows, fa + e[:, 3], first[e[:, 0]] + e[:, 1] + e[:, 3], e[:, 4])
        for (b, d, v, lo, m), sc in zip(elig, scores):
            cur = best.get(b)
            if cur is None or sc > cur[3] or (sc == cur[3] and d < cur[0]):
                best[b] = (d, lo, m, sc, v)
    ranked = sorted(best.items(), key=lambda kv: (-kv[1][3], kv[0]))[:top]
    return [(b, d, lo, m, sc, v) for b, (d, lo, m, sc, v) in ranked]


def self_match_ref(index_rows, first, ids, tracks=None, top=8, min_votes=4, min_overlap=1):
    """All source tracks (default: every track) -> (b, delta, i_lo, m, score, votes) arrays (n_src, top), padded like the
    kernel with -1 / INT_MIN / -1 / 0 / -inf / 0."""
    T = len(first) - 1
    tracks = list(range(T)) if tracks is None else [int(t) for t in tracks]
    ns = len(tracks)
    b_ = np.full((ns, top), -1, np.int32)
    d_ = np.full((ns, top), np.iinfo(np.int32).min, np.int32)
    lo_ = np.full((ns, top), -1, np.int32)
    m_ = np.zeros((ns, top), np.int32)
    sc_ = np.full((ns, top), -np.inf, np.float32)
    v_ = np.zeros((ns, top), np.int32)
    for s, a in enumerate(tracks):
        for j, (b, d, lo, m, sc, v) in enumerate(self_match_track(index_rows, first, ids, a, top, min_votes,
                                                                  min_overlap)):
            b_[s, j], d_[s, j], lo_[s, j], m_[s, j], sc_[s, j], v_[s, j] = b, d, lo, m, sc, v
    return b_, d_, lo_, m_, sc_, v_
