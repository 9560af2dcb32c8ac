"""numpy restatement of grafp_identify_f32 (csrc/identify.hip, include/grafp_hip.h): the contract the kernel is tested
against.  fmaf is emulated with an exact float64 product and a rounding to f32 after every step; the 32 lane sums are
combined by the butterfly 16, 8, 4, 2, 1 and the score is one f32 division."""
import numpy as np


def score_runs(q, rows, q_lo, r_lo, o):
    """score_run for many runs at once: run c is q[q_lo[c] : q_lo[c] + o[c]] against rows[r_lo[c] : r_lo[c] + o[c]]
    (o[c] >= 1).  Every run gets its own chain; steps past a run's length leave its lanes alone."""
    q_lo, r_lo, o = (np.asarray(v, np.int64) for v in (q_lo, r_lo, o))
    acc = np.zeros((len(o), 32), np.float32)
    for i in range(int(o.max(initial=0))):
        live = (i < o)[:, None]
        qi = np.asarray(q, np.float32)[np.minimum(q_lo + i, len(q) - 1)]
        ri = np.asarray(rows, np.float32)[np.minimum(r_lo + i, len(rows) - 1)]
        for e in range(4):
            prod = qi[:, e::4].astype(np.float64) * ri[:, e::4].astype(np.float64)        # lane l: dim 4l + e
            acc = np.where(live, (prod + acc.astype(np.float64)).astype(np.float32), acc)
    for sh in (16, 8, 4, 2, 1):
        acc = (acc + acc[:, np.arange(32) ^ sh]).astype(np.float32)
    return (acc[:, 0] / o.astype(np.float32)).astype(np.float32)


def score_run(q, rows):
    """Mean dot product of q (o, 128) and rows (o, 128) in the kernel's arithmetic order."""
    return score_runs(q, rows, [0], [0], [len(q)])[0]


def identify_item(index_rows, first, q, ids, top=5, min_overlap=None):
    """One item: q (ql, 128) query rows, ids (ql, k) library ids.  -> list of (track, offset, score, votes), best first."""
    index_rows = np.asarray(index_rows, np.float32)
    first = np.asarray(first, np.int64)
    n, T = index_rows.shape[0], first.shape[0] - 1
    ql = q.shape[0]
    need_q = ql if min_overlap is None else int(min_overlap)
    votes = {}
    for s in range(ql):
        for r in np.asarray(ids[s]).tolist():
            if 0 <= r < n:
                t = int(np.searchsorted(first, r, side="right")) - 1
                t = min(t, T - 1)
                key = (t, r - s)
                votes[key] = votes.get(key, 0) + 1
    cands = []
    for (t, a), v in votes.items():
        f0, f1 = int(first[t]), int(first[t + 1])
        lo, hi = max(0, f0 - a), min(ql, f1 - a)
        o = hi - lo
        if o >= 1 and o >= min(need_q, f1 - f0):
            cands.append((t, a, v, lo, o))
    best = {}
    if cands:
        c = np.array(cands, np.int64)
        scores = score_runs(q, index_rows, c[:, 3], c[:, 1] + c[:, 3], c[:, 4])
        for (t, a, v, _, _), sc in zip(cands, scores):
            cur = best.get(t)
            if cur is None or sc > cur[1] or (sc == cur[1] and a < cur[0]):
                best[t] = (a, sc, v)
    ranked = sorted(best.items(), key=lambda kv: (-kv[1][1], kv[0]))[:top]
    return [(t, a - int(first[t]), sc, v) for t, (a, sc, v) in ranked]


def identify_ref(index_rows, first, q_rows, topk_ids, item_row, item_len, top=5, min_overlap=None):
    """All items -> (track, offset, score, votes) arrays (n_items, top), padded like the kernel."""
    n_items = len(item_row)
    tr = np.full((n_items, top), -1, np.int32)
    off = np.full((n_items, top), np.iinfo(np.int32).min, np.int32)
    sc = np.full((n_items, top), -np.inf, np.float32)
    vo = np.zeros((n_items, top), np.int32)
    for i in range(n_items):
        r0, ql = int(item_row[i]), int(item_len[i])
        res = identify_item(index_rows, first, np.asarray(q_rows[r0:r0 + ql]), np.asarray(topk_ids[r0:r0 + ql]), top,
                            min_overlap)
        for j, (t, o, s, v) in enumerate(res):
            tr[i, j], off[i, j], sc[i, j], vo[i, j] = t, o, s, v
    return tr, off, sc, vo
