"""numpy restatement of the merge of a sharded library's lists (csrc/merge_lists.hip, ops.merge_track_lists), and the
random lists the CPU and GPU tests feed it."""
import numpy as np

OVERFLOW = -2                                  # cross_match's mark of a source that did not fit its workspace


def merge_ref(track, score, payload, track_base, pad):
    """track (S, n_items, top) int32 shard-local (negative: padding), score (S, n_items, top) f32, payload
    (P, S, n_items, top) int32, track_base S ints, pad P ints -> (track (n_items, top) global, score, payload
    (P, n_items, top)): per item the non-padding entries by score descending, then global track ascending, the first
    `top` of them; the rest -1 / -inf / pad[p].  Any entry -2: slot 0 gets -2, everything else is padding."""
    track, score, payload = np.asarray(track, np.int32), np.asarray(score, np.float32), np.asarray(payload, np.int32)
    S, n_items, top = track.shape
    P = payload.shape[0]
    out_t = np.full((n_items, top), -1, np.int32)
    out_s = np.full((n_items, top), -np.inf, np.float32)
    out_p = np.empty((P, n_items, top), np.int32)
    for p in range(P):
        out_p[p] = pad[p]
    for i in range(n_items):
        if (track[:, i] == OVERFLOW).any():
            out_t[i, 0] = OVERFLOW
            continue
        entries = [(-float(score[s, i, j]), int(track_base[s]) + int(track[s, i, j]), s, j)
                   for s in range(S) for j in range(top) if track[s, i, j] >= 0]
        entries.sort(key=lambda e: e[:2])
        for r, (neg, t, s, j) in enumerate(entries[:top]):
            out_t[i, r], out_s[i, r] = t, score[s, i, j]
            out_p[:, i, r] = payload[:, s, i, j]
    return out_t, out_s, out_p


def random_lists(seed, S, n_items, top, P, tracks_per_shard=9, keep=1.0, levels=4):
    """Lists as the shards' ops write them: per (shard, item) up to `top` distinct local tracks (each kept with
    probability `keep`, then padding), scores drawn from `levels` values so that ties occur inside and across shards, in
    the ops' own order (score descending, track ascending); random payloads.  -> (track, score, payload, track_base,
    pad)."""
    rng = np.random.RandomState(seed)
    pad = [[-2 ** 31, 0, -1, 0, 0, 7][p] for p in range(P)]
    track = np.full((S, n_items, top), -1, np.int32)
    score = np.full((S, n_items, top), -np.inf, np.float32)
    payload = np.empty((P, S, n_items, top), np.int32)
    for p in range(P):
        payload[p] = pad[p]
    sizes = rng.randint(0, tracks_per_shard + 1, size=S)
    sizes[0] = tracks_per_shard
    track_base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
    values = (np.arange(levels, dtype=np.float32) - 1.0) / 4.0              # -0.25, 0, 0.25, ...
    for s in range(S):
        for i in range(n_items):
            m = min(top, int(sizes[s]))
            m = int((rng.rand(m) < keep).sum())
            t = rng.choice(int(sizes[s]), size=m, replace=False) if m else np.zeros(0, np.int64)
            sc = values[rng.randint(0, levels, size=m)]
            order = np.lexsort((t, -sc))
            track[s, i, :m], score[s, i, :m] = t[order], sc[order]
            payload[:, s, i, :m] = rng.randint(-1000, 1000, size=(P, m))
    return track, score, payload, track_base, pad
