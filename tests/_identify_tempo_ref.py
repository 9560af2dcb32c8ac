"""numpy restatement of grafp_identify_tempo_f32 (csrc/identify_tempo.hip, include/grafp_hip.h): identification of
recordings that play faster or slower than the catalogue.  A ratio is an integer num in [128, 512] standing for num / 256;
query row s sits w(s) = (s * num + 128) >> 8 library rows after query row 0.  The score of a candidate is
_identify_ref.score_runs over its pairs, the library rows gathered in s order."""
import numpy as np

from _identify_ref import score_runs


def w(s, num):
    """Rows after query row 0 at which query row s sits at ratio num / 256 (integer arithmetic, as the kernel's)."""
    return (np.asarray(s, np.int64) * int(num) + 128) >> 8


def pairs_of(a, f0, f1, ql, num):
    """The query rows s of alignment a at ratio num whose library row a + w(s) lies inside the track [f0, f1)."""
    return [s for s in range(ql) if f0 <= a + int(w(s, num)) < f1]


def prefer(num):
    """Sort key of the ratio tie rule: nearer to 1 first, then the smaller ratio."""
    return (abs(int(num) - 256), int(num))


def tempo_item(index_rows, first, q, ids, ratio_num, top=5, min_overlap=None):
    """One item: q (ql, 128) query rows, ids (ql, k) library ids.  -> list of (track, offset, score, votes, num), best
    first."""
    index_rows = np.asarray(index_rows, np.float32)
    first = np.asarray(first, np.int64)
    n, T = index_rows.shape[0], first.shape[0] - 1
    ql = q.shape[0]
    need = ql if min_overlap is None else int(min_overlap)
    cands, q_parts, r_parts, q_lo, os_ = [], [], [], [], []
    at = 0
    for num in (int(v) for v in ratio_num):
        votes = {}
        for s in range(ql):
            for r in np.asarray(ids[s]).tolist():
                if 0 <= r < n:
                    t = min(int(np.searchsorted(first, r, side="right")) - 1, T - 1)
                    key = (t, r - int(w(s, num)))
                    votes[key] = votes.get(key, 0) + 1
        for (t, a), v in votes.items():
            f0, f1 = int(first[t]), int(first[t + 1])
            p = pairs_of(a, f0, f1, ql, num)
            o = len(p)
            if o >= 1 and o >= min(need, max(1, ((f1 - f0) * 256) // num)):
                assert p == list(range(p[0], p[0] + o))                  # w never decreases: a contiguous range of s
                cands.append((t, a, v, num))
                q_parts.append(np.asarray(q, np.float32)[p])
                r_parts.append(index_rows[a + w(p, num)])
                q_lo.append(at)
                os_.append(o)
                at += o
    best = {}
    if cands:
        scores = score_runs(np.concatenate(q_parts), np.concatenate(r_parts), q_lo, q_lo, os_)
        for (t, a, v, num), sc in zip(cands, scores):
            cur = best.get(t)
            if cur is None or sc > cur[1] or (sc == cur[1] and (prefer(num), a) < (prefer(cur[3]), cur[0])):
                best[t] = (a, sc, v, num)
    ranked = sorted(best.items(), key=lambda kv: (-kv[1][1], kv[0]))[:top]
    return [(t, a - int(first[t]), sc, v, num) for t, (a, sc, v, num) in ranked]


def tempo_ref(index_rows, first, q_rows, topk_ids, item_row, item_len, ratio_num, top=5, min_overlap=None):
    """All items -> (track, offset, score, votes, ratio) arrays (n_items, top), padded like the kernel."""
    n_items = len(item_row)
    tr = np.full((n_items, top), -1, np.int32)
    off = np.full((n_items, top), np.iinfo(np.int32).min, np.int32)
    sc = np.full((n_items, top), -np.inf, np.float32)
    vo = np.zeros((n_items, top), np.int32)
    ra = np.zeros((n_items, top), np.int32)
    for i in range(n_items):
        r0, ql = int(item_row[i]), int(item_len[i])
        res = tempo_item(index_rows, first, np.asarray(q_rows[r0:r0 + ql]), np.asarray(topk_ids[r0:r0 + ql]),
                         ratio_num, top, min_overlap)
        for j, (t, o, s, v, num) in enumerate(res):
            tr[i, j], off[i, j], sc[i, j], vo[i, j], ra[i, j] = t, o, s, v, num
    return tr, off, sc, vo, ra


def tempo_case(seed, ratio_num, n_items=64, max_ql=40, k=6):
    """Dyadic rows (multiples of 2^-8 in [-1/16, 1/16): every sum is exact) over 24 tracks of 0 to 60 rows (zero-length
    ones and a 3-row one included, track 3 a copy of track 1); items of 0 to max_ql rows planted at random positions --
    hanging over a track's ends too -- and random ratios of ratio_num, whose hits go to the planted row and to its
    neighbours, with duplicate, random and -1 ids around them.  -> (rows, first, q, ids, item_row, item_len)."""
    rng = np.random.RandomState(seed)
    ratio_num = [int(v) for v in ratio_num]
    lens = rng.randint(0, 61, size=24)
    lens[[0, 7]] = 0
    lens[2] = 3
    lens[1] = lens[3] = 40
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(first[-1])
    rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
    rows[first[3]:first[4]] = rows[first[1]:first[2]]
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
        num = ratio_num[rng.randint(len(ratio_num))]
        p0 = rng.randint(-(ql // 2), lens[t] - ql // 2 + 1)           # the row of query row 0 in track t
        for s in range(ql):
            p = p0 + int(w(s, num))
            if 0 <= p < lens[t]:
                r = int(first[t]) + p
                if rng.rand() < 0.8:
                    q[r0 + s] = rows[r]
                ids[r0 + s, 0] = r
                if r + 1 < n:
                    ids[r0 + s, 1] = r + 1                           # the neighbours, across a track's end too
                if r >= 1 and k > 3:
                    ids[r0 + s, 3] = r - 1
                if rng.rand() < 0.2:
                    ids[r0 + s, 2] = r                               # a duplicate hit
    return rows, first, q, ids, item_row, item_len
