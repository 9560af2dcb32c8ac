"""numpy restatement of grafp_identify_thin_f32 (csrc/identify_thin.hip, include/grafp_hip.h): identification against a
library that keeps every D-th fingerprint row of each track.  Library row j of track t is the track's dense segment
j * D; the query stays dense.  The score of a candidate is _identify_ref.score_runs over its pairs gathered in s order
(the query steps D rows per pair, the library one)."""
import numpy as np

from _identify_ref import score_runs


def thin_first(first, D):
    """The track table of the thinned library: a track of S dense rows keeps ceil(S / D)."""
    lens = np.diff(np.asarray(first, np.int64))
    return np.concatenate([[0], np.cumsum(-(-lens // D))]).astype(np.int64)


def thin_rows(rows, first, D):
    """Rows first[t] + 0, D, 2D, ... of every track of a dense library -> (kept rows, their track table)."""
    first = np.asarray(first, np.int64)
    keep = [np.arange(first[t], first[t + 1], D) for t in range(len(first) - 1)]
    keep = np.concatenate(keep).astype(np.int64) if keep else np.zeros(0, np.int64)
    return np.asarray(rows)[keep], thin_first(first, D)


def pairs_of(a, f0, f1, ql, D):
    """The query rows s of candidate alignment a that sit on a kept row of the track [f0, f1): ascending."""
    return [s for s in range(ql) if (a + s) % D == 0 and f0 <= (a + s) // D < f1]


def thin_item(index_rows, first, q, ids, D, top=5, min_overlap=None):
    """One item: q (ql, 128) dense query rows, ids (ql, k) ids of kept rows.  -> list of (track, offset, score, votes),
    best first; offset in dense segments from the track's start."""
    index_rows = np.asarray(index_rows, np.float32)
    first = np.asarray(first, np.int64)
    D = int(D)
    n, T = index_rows.shape[0], first.shape[0] - 1
    ql = q.shape[0]
    need_q = ql if min_overlap is None else int(min_overlap)
    need = max(1, need_q // D)
    votes = {}
    for s in range(ql):
        for r in np.asarray(ids[s]).tolist():
            if 0 <= r < n:
                t = min(int(np.searchsorted(first, r, side="right")) - 1, T - 1)
                key = (t, r * D - s)
                votes[key] = votes.get(key, 0) + 1
    cands, q_parts, q_lo, r_lo, os_ = [], [], [], [], []
    at = 0
    for (t, a), v in votes.items():
        f0, f1 = int(first[t]), int(first[t + 1])
        p = pairs_of(a, f0, f1, ql, D)
        o = len(p)
        if o >= 1 and o >= min(need, f1 - f0):
            assert p == list(range(p[0], p[0] + o * D, D))
            cands.append((t, a, v))
            q_parts.append(np.asarray(q, np.float32)[p])
            q_lo.append(at)
            r_lo.append((a + p[0]) // D)
            os_.append(o)
            at += o
    best = {}
    if cands:
        scores = score_runs(np.concatenate(q_parts), index_rows, q_lo, r_lo, os_)
        for (t, a, v), sc in zip(cands, scores):
            cur = best.get(t)
            if cur is None or sc > cur[1] or (sc == cur[1] and a < cur[0]):
                best[t] = (a, sc, v)
    ranked = sorted(best.items(), key=lambda kv: (-kv[1][1], kv[0]))[:top]
    return [(t, a - int(first[t]) * D, sc, v) for t, (a, sc, v) in ranked]


def thin_ref(index_rows, first, q_rows, topk_ids, item_row, item_len, D, top=5, min_overlap=None):
    """All items -> (track, offset, score, votes) arrays (n_items, top), padded like the kernel."""
    n_items = len(item_row)
    tr = np.full((n_items, top), -1, np.int32)
    off = np.full((n_items, top), np.iinfo(np.int32).min, np.int32)
    sc = np.full((n_items, top), -np.inf, np.float32)
    vo = np.zeros((n_items, top), np.int32)
    for i in range(n_items):
        r0, ql = int(item_row[i]), int(item_len[i])
        res = thin_item(index_rows, first, np.asarray(q_rows[r0:r0 + ql]), np.asarray(topk_ids[r0:r0 + ql]), D, top,
                        min_overlap)
        for j, (t, o, s, v) in enumerate(res):
            tr[i, j], off[i, j], sc[i, j], vo[i, j] = t, o, s, v
    return tr, off, sc, vo


def thin_case(seed, D, n_items=96, max_ql=40, k=6):
    """Dyadic rows (multiples of 2^-8 in [-1/16, 1/16): every sum is exact) over 24 dense tracks of 0 to 60 * D segments
    (zero-length ones and a 3-segment one included, track 3 a copy of track 1), thinned to every D-th row; queries
    planted at random fine positions -- hanging over a track's ends too -- whose hits go to the kept row at or before
    each planted position and to the next kept row, with duplicate, random and -1 ids around them.
    -> (kept rows, their track table, q, ids, item_row, item_len)."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, 60 * D + 1, size=24)
    lens[[0, 7]] = 0
    lens[2] = 3
    lens[1] = lens[3] = 40 * D
    dfirst = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dense = (rng.randint(-16, 16, size=(int(dfirst[-1]), 128)) / 256.0).astype(np.float32)
    dense[dfirst[3]:dfirst[4]] = dense[dfirst[1]:dfirst[2]]
    rows, first = thin_rows(dense, dfirst, D)
    n = rows.shape[0]
    item_len = rng.randint(1, max_ql + 1, size=n_items).astype(np.int32)
    item_len[0] = 0
    item_row = np.concatenate([[0], np.cumsum(item_len[:-1])]).astype(np.int64)
    nq = int(item_len.sum())
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = rng.randint(-1, n, size=(nq, k)).astype(np.int64)
    full = np.flatnonzero(lens > 0)
    for i in range(n_items):
        ql, r0 = int(item_len[i]), int(item_row[i])
        t = int(full[rng.randint(len(full))])
        p0 = rng.randint(-(ql // 2), lens[t] - ql // 2 + 1)           # the fine position of query row 0 in track t
        for s in range(ql):
            p = p0 + s
            if 0 <= p < lens[t]:
                if rng.rand() < 0.8:
                    q[r0 + s] = dense[dfirst[t] + p]
                r = int(first[t]) + p // D
                ids[r0 + s, 0] = r                                   # the kept row at or before the position
                if r + 1 < first[t + 1]:
                    ids[r0 + s, 1] = r + 1                           # and the next one
                if rng.rand() < 0.2:
                    ids[r0 + s, 2] = r                               # a duplicate hit
    return rows, first, q, ids, item_row, item_len
