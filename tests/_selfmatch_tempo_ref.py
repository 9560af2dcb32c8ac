"""numpy restatement of grafp_self_match_tempo_f32 (csrc/selfmatch_tempo.hip, include/grafp_hip.h): tracks of a library
that share audio at another speed.  A thin layer over _crossmatch_tempo_ref, so the two restatements cannot drift apart:
the sources are the source tracks' own rows laid end to end, their hits the rows' hits with every hit inside the source's
own track replaced by -1 (as_cross_match), and everything else -- votes, spans, scores, the tie rule, the padding -- is
cross_match_tempo_ref's.  library_case / short_case build libraries of dyadic rows with copies planted between tracks along
a slope, hits in both directions."""
import numpy as np

from _crossmatch_tempo_ref import cross_match_tempo_ref, eligible_candidates
from _identify_tempo_ref import w


def as_cross_match(index_rows, first, ids, tracks=None, mask=True):
    """The cross-match form of a self-match call -> (q_rows, src_first, topk_ids): the source tracks' own rows laid end
    to end, the table of their row counts, and those rows' hits, own-track hits replaced by -1 (mask=False: kept)."""
    index_rows, ids = np.asarray(index_rows, np.float32), np.asarray(ids, np.int64)
    first = np.asarray(first, np.int64)
    tracks = list(range(len(first) - 1)) if tracks is None else [int(t) for t in tracks]
    g = [np.arange(first[t], first[t + 1]) for t in tracks]
    src_first = np.concatenate([[0], np.cumsum([len(x) for x in g])]).astype(np.int64)
    g = np.concatenate(g + [np.zeros(0, np.int64)]).astype(np.int64)
    q, hit = index_rows[g], ids[g].copy()
    if mask:
        for s, t in enumerate(tracks):
            own = hit[src_first[s]:src_first[s + 1]]
            own[(own >= first[t]) & (own < first[t + 1])] = -1
    return q, src_first, hit


def self_match_tempo_ref(index_rows, first, ids, ratio_num, tracks=None, top=8, min_votes=4, min_overlap=1):
    """All source tracks (default: every track) -> (b, delta, i_lo, m, score, votes, ratio) arrays (n_src, top), padded
    like the kernel with -1 / INT_MIN / -1 / 0 / -inf / 0 / 0."""
    q, src_first, hit = as_cross_match(index_rows, first, ids, tracks)
    return cross_match_tempo_ref(index_rows, first, q, src_first, hit, ratio_num, top, min_votes, min_overlap)


def eligible_of_track(index_rows, first, ids, a, ratio_num, min_votes=4, min_overlap=1):
    """Source track a -> int64 arrays (b, a_g, num, votes, i_lo, m) of its eligible candidates over all ratios."""
    _, _, hit = as_cross_match(index_rows, first, ids, [a])
    return eligible_candidates(len(index_rows), first, hit, ratio_num, min_votes, min_overlap)


def library_case(seed, lens, k, plants, p_random=0.3, same_tracks=(), repeats=(), p_hit=0.9, p_back=0.7):
    """A library of dyadic rows (multiples of 2^-8 in [-1/16, 1/16): every sum is exact) over tracks of lens rows and the
    hits (n, k) of its rows.  same_tracks (dst, src): tracks with equal rows.  repeats: tracks whose second half is their
    first half again, every row hitting its twin (own-track hits: no hits).  `plants` (track a, row in it, global library
    row, length, num) copy rows of other tracks into a ALONG THE SLOPE of ratio num: row i of a takes library row g0 +
    w(i) - w(off), which may run across a partner's end (rows past the library's end or inside a itself are left alone);
    every planted row hits the row it copies with probability p_hit, sometimes twice, and is hit BY it with probability
    p_back (the other direction, along the inverse slope); the other ids are random (own track included), -1 or out of
    range.  -> (rows, first, ids)."""
    rng = np.random.RandomState(seed)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(first[-1])
    rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
    for dst, src in same_tracks:
        rows[first[dst]:first[dst + 1]] = rows[first[src]:first[src + 1]]
    ids = np.where(rng.rand(n, k) < p_random, rng.randint(0, n, size=(n, k)), -1).astype(np.int64)
    for t in repeats:
        f, half = int(first[t]), int(lens[t]) // 2
        rows[f + half:f + 2 * half] = rows[f:f + half]
        ids[f:f + half, 0] = np.arange(f + half, f + 2 * half)
        ids[f + half:f + 2 * half, 0] = np.arange(f, f + half)
    for a, off, g0, ln, num in plants:
        fa, fb = int(first[a]), int(first[a + 1])
        assert off + ln <= fb - fa, (a, off, ln)
        for i in range(off, off + ln):
            r = g0 + int(w(i, num)) - int(w(off, num))
            if not 0 <= r < n or fa <= r < fb:
                continue
            rows[fa + i] = rows[r]
            if rng.rand() < p_hit:
                ids[fa + i, rng.randint(k)] = r
            if rng.rand() < 0.1:
                ids[fa + i, rng.randint(k)] = r                        # a duplicate hit, or one that replaces the first
            if rng.rand() < p_back:
                ids[r, rng.randint(k)] = fa + i
    ids[rng.rand(n, k) < 0.02] = -5                                    # out of range: no hit
    ids[rng.rand(n, k) < 0.01] = n + 3
    return rows, first, ids


REPEATING = 6                         # short_case's track that repeats itself


def short_case(seed, k, ratio_num):
    """About 60 tracks of 0..70 rows: zero-row and one-row tracks, two equal tracks (4 and 5), one that repeats itself
    (REPEATING), three plants across a partner's end, and 40 plants of 4 to 40 rows along ratios drawn from ratio_num."""
    rng = np.random.RandomState(seed)
    ratio_num = [int(v) for v in ratio_num]
    lens = rng.randint(0, 71, size=60)
    lens[[0, 9, 10]] = 0
    lens[[2, 8]] = 1
    lens[[4, 5]] = 64
    lens[REPEATING] = 60
    lens[[3, 7]] = 70
    for t in (12, 30, 44):
        lens[t], lens[t + 1] = max(lens[t], 10), max(lens[t + 1], 10)
    first = np.concatenate([[0], np.cumsum(lens)])
    n = int(first[-1])
    pick = lambda: ratio_num[rng.randint(len(ratio_num))]
    plants = [(5, 0, int(first[4]), 64, 256), (3, 0, int(first[20]), 30, pick()), (8, 0, int(first[21]), 1, pick())]
    for t in (12, 30, 44):                                                      # across the end of track t
        plants.append((3 if t == 12 else 7, 40 if t != 30 else 50, int(first[t + 1]) - 3, 8, pick()))
    for _ in range(40):
        a = int(rng.choice(np.setdiff1d(np.flatnonzero(lens >= 8), [4, 5, REPEATING])))   # (those keep their rows)
        ln = int(rng.randint(4, min(lens[a], 40) + 1))
        plants.append((a, int(rng.randint(0, lens[a] - ln + 1)), int(rng.randint(0, n - 2 * ln)), ln, pick()))
    return library_case(seed + 1, lens, k, plants, same_tracks=[(5, 4)], repeats=[REPEATING])
