"""numpy restatement of grafp_cross_match_tempo_f32 (csrc/crossmatch_tempo.hip, include/grafp_hip.h): what recordings
that play faster or slower than the catalogue share with a library.  A ratio is an integer num in [128, 512] standing for
num / 256; row i of a source (counted from the source's row 0) sits w(i) = (i * num + 128) >> 8 library rows after the
source's row 0.  The score of a candidate is _identify_ref.score_runs over its span, the library rows gathered in i order.
The hit-to-track lookup is one searchsorted over all hits of a source and the grouping one lexsort per ratio, so a source
of thousands of rows costs seconds."""
import numpy as np

from _identify_ref import score_runs
from _identify_tempo_ref import prefer, w

INT_MIN = np.iinfo(np.int32).min


def wv(i, num):
    """w for arrays of rows and of ratios."""
    return (np.asarray(i, np.int64) * np.asarray(num, np.int64) + 128) >> 8


def eligible_candidates(n, first, ids, ratio_num, min_votes=4, min_overlap=1):
    """One source, ids (L, k) the hits of its rows -> int64 arrays (b, a, num, votes, i_lo, m) of its eligible candidates
    over all ratios.  Nothing is dropped but ids outside [0, n)."""
    first = np.asarray(first, np.int64)
    ids = np.asarray(ids, np.int64)
    T = first.shape[0] - 1
    L, k = ids.shape
    i_all = np.repeat(np.arange(L, dtype=np.int64), k)
    r_all = ids.reshape(-1)
    ok = (r_all >= 0) & (r_all < n)
    i_all, r_all = i_all[ok], r_all[ok]
    parts = [[np.zeros(0, np.int64)] for _ in range(6)]
    if r_all.size:
        b_all = np.minimum(np.searchsorted(first, r_all, side="right") - 1, T - 1)
        for num in (int(v) for v in ratio_num):
            a_all = r_all - wv(i_all, num)
            order = np.lexsort((i_all, a_all, b_all))                 # by partner, then alignment, then row
            b, a, i = b_all[order], a_all[order], i_all[order]
            st = np.flatnonzero(np.concatenate([[True], (b[1:] != b[:-1]) | (a[1:] != a[:-1])]))
            en = np.concatenate([st[1:], [b.size]])
            votes, i_lo, m = en - st, i[st], i[en - 1] - i[st] + 1
            keep = (votes >= min_votes) & (m >= min_overlap)
            for p, v in zip(parts, (b[st], a[st], np.full(st.size, num, np.int64), votes, i_lo, m)):
                p.append(v[keep])
    return tuple(np.concatenate(p) for p in parts)


def score_candidates(q, index_rows, a, num, i_lo, m, chunk=4096, chunk_rows=1 << 18):
    """The scores of spans [i_lo, i_lo + m) at alignment a and ratio num (arrays), in chunks of similar length (at most
    `chunk` spans and about chunk_rows gathered rows each)."""
    q, index_rows = np.asarray(q, np.float32), np.asarray(index_rows, np.float32)
    out = np.zeros(len(m), np.float32)
    order = np.argsort(m, kind="stable")
    c0 = 0
    while c0 < len(order):
        c1 = min(c0 + chunk, len(order))
        ms = m[order[c0:c1]]                                            # ascending; score_runs walks the longest
        c1 = max(c0 + 1, c0 + min(int(np.searchsorted(np.cumsum(ms), chunk_rows, side="right")),
                                  int(np.searchsorted(ms, 2 * ms[0] + 8, side="right"))))
        c, c0 = order[c0:c1], c1
        mm = m[c]
        offs = np.cumsum(mm) - mm
        t = np.arange(int(mm.sum()), dtype=np.int64) - np.repeat(offs, mm)
        qi = np.repeat(i_lo[c], mm) + t
        ri = np.repeat(a[c], mm) + wv(qi, np.repeat(num[c], mm))
        assert ri.min() >= 0 and ri.max() < len(index_rows)
        out[c] = score_runs(q[qi], index_rows[ri], offs, offs, mm)
    return out


def cross_match_tempo_source(index_rows, first, q, ids, ratio_num, top=8, min_votes=4, min_overlap=1):
    """One source -> list of (b, delta, i_lo, m, score, votes, num), best first."""
    first = np.asarray(first, np.int64)
    b, a, num, votes, i_lo, m = eligible_candidates(len(index_rows), first, ids, ratio_num, min_votes, min_overlap)
    best = {}
    if b.size:
        # every row of a span lies in its partner: w never decreases and the two end rows do
        assert (a + wv(i_lo, num) >= first[b]).all() and (a + wv(i_lo + m - 1, num) < first[b + 1]).all()
        scores = score_candidates(q, index_rows, a, num, i_lo, m)
        for c in range(b.size):
            key = (-scores[c], prefer(num[c]), int(a[c]))
            cur = best.get(int(b[c]))
            if cur is None or key < cur[0]:
                best[int(b[c])] = (key, c)
    ranked = sorted(best.items(), key=lambda kv: (kv[1][0][0], kv[0]))[:top]
    return [(t, int(a[c]) - int(first[t]), int(i_lo[c]), int(m[c]), scores[c], int(votes[c]), int(num[c]))
            for t, (_, c) in ranked]


def cross_match_tempo_ref(index_rows, first, q_rows, src_first, ids, ratio_num, top=8, min_votes=4, min_overlap=1):
    """All sources -> (b, delta, i_lo, m, score, votes, ratio) arrays (S, top), padded like the kernel with
    -1 / INT_MIN / -1 / 0 / -inf / 0 / 0."""
    q_rows, ids = np.asarray(q_rows, np.float32), np.asarray(ids, np.int64)
    src_first = np.asarray(src_first, np.int64)
    ns = len(src_first) - 1
    pad = (-1, INT_MIN, -1, 0, -np.inf, 0, 0)
    outs = [np.full((ns, top), pad[j], np.float32 if j == 4 else np.int32) for j in range(7)]
    for s in range(ns):
        r0, r1 = int(src_first[s]), int(src_first[s + 1])
        for j, res in enumerate(cross_match_tempo_source(index_rows, first, q_rows[r0:r1], ids[r0:r1], ratio_num, top,
                                                         min_votes, min_overlap)):
            for o, v in zip(outs, res):
                o[s, j] = v
    return tuple(outs)


def tempo_match_case(seed, lib_lens, src_lens, k, plants, p_random=0.3, same_tracks=(), p_hit=0.9):
    """A library of dyadic rows (multiples of 2^-8 in [-1/16, 1/16): every sum is exact) over tracks of lib_lens rows,
    and sources of src_lens random rows outside it.  `plants` (source, row in it, global library row, length, num) copy
    library rows into a source ALONG THE SLOPE of ratio num: source row i takes library row g0 + w(i) - w(off), which may
    run across a track's end (rows past the library's end stay random); every planted row hits the row it copies with
    probability p_hit, sometimes twice; the other ids are random, -1 or out of range.  same_tracks (dst, src): library
    tracks with equal rows.  -> (rows, first, q, src_first, ids)."""
    rng = np.random.RandomState(seed)
    first = np.concatenate([[0], np.cumsum(lib_lens)]).astype(np.int64)
    n = int(first[-1])
    rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
    for dst, src in same_tracks:
        rows[first[dst]:first[dst + 1]] = rows[first[src]:first[src + 1]]
    src_first = np.concatenate([[0], np.cumsum(src_lens)]).astype(np.int64)
    nq = int(src_first[-1])
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = np.where(rng.rand(nq, k) < p_random, rng.randint(0, n, size=(nq, k)), -1).astype(np.int64)
    for s, off, g0, ln, num in plants:
        q0 = int(src_first[s])
        assert off + ln <= src_lens[s], (s, off, ln)
        for i in range(off, off + ln):
            r = g0 + int(w(i, num)) - int(w(off, num))
            if not 0 <= r < n:
                continue
            q[q0 + i] = rows[r]
            if rng.rand() < p_hit:
                ids[q0 + i, rng.randint(k)] = r
            if rng.rand() < 0.1:
                ids[q0 + i, rng.randint(k)] = r                        # a duplicate hit, or one that replaces the first
    ids[rng.rand(nq, k) < 0.02] = -5                                   # out of range: no hit
    ids[rng.rand(nq, k) < 0.01] = n + 3
    return rows, first, q, src_first, ids


def short_case(seed, k, ratio_num):
    """About 60 library tracks and 60 sources of 0..70 rows (zero-row and one-row ones included, two equal library
    tracks), 40 plants of 4 to 40 rows along ratios drawn from ratio_num, three across a track's end, and short plants at
    source row 0 on which neighbouring ratios read the same rows (equal scores: the ratio tie rule)."""
    rng = np.random.RandomState(seed)
    ratio_num = [int(v) for v in ratio_num]
    lib_lens = rng.randint(0, 70, size=60)
    lib_lens[[0, 9, 10]] = 0
    lib_lens[[4, 5]] = 64
    lib_lens[2] = 1
    src_lens = rng.randint(0, 71, size=60)
    src_lens[[0, 7, 59]] = 0
    src_lens[[1, 8]] = 1
    src_lens[[3, 4]] = 70
    first = np.concatenate([[0], np.cumsum(lib_lens)])
    n = int(first[-1])
    pick = lambda: ratio_num[rng.randint(len(ratio_num))]
    plants = [(3, 0, int(first[4]), 30, pick()), (4, 6, int(first[5]), 30, pick()),      # tracks 4 and 5 are equal
              (1, 0, int(first[20]), 1, pick())]
    for t in (12, 30, 44):                                                      # across the end of track t
        plants.append((3 if t == 12 else 4, 40 if t != 30 else 50, int(first[t + 1]) - 3, 8, pick()))
    for s in np.flatnonzero(src_lens >= 8)[:6]:                                 # the same rows at neighbouring ratios
        plants.append((int(s), 0, int(rng.randint(0, n - 8)), 6, pick()))
    for _ in range(40):
        s = int(rng.choice(np.flatnonzero(src_lens >= 8)))
        ln = int(rng.randint(4, min(src_lens[s], 40) + 1))
        plants.append((s, int(rng.randint(0, src_lens[s] - ln + 1)), int(rng.randint(0, n - 2 * ln)), ln, pick()))
    return tempo_match_case(seed + 1, lib_lens, src_lens, k, plants, same_tracks=[(5, 4)])
