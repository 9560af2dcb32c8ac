"""Measurements of shared-audio detection inside a library (ops.self_match, csrc/selfmatch.hip) and, with --cross, of
whole recordings against it (ops.cross_match / cross_match_pq, csrc/crossmatch.hip); prints one JSON line.

A library of --tracks tracks x --track-s seconds (default 3 300 x 30 s: 303 segments each, about 1 M rows of random unit
fingerprints) with --copies planted copies (default 100): a noisy sub-range of one track written into another at a known
offset.  Then:
  search      ops.FlatL2Index.search of every library row against the library at k = --k (default 32), the self-search
  self_match  ops.self_match of all tracks in one launch (top 8, min_votes 4)
  recall      planted pairs found in both directions with the exact offset
Times from events (median of --reps); `rocprofv3 --kernel-trace --stats -- python tools/selfmatch_bench.py` gives the
per-kernel figures.  Target: self_match <= 0.25 x search.
--cross: the sources are copies of the library's tracks held outside the library, their hits the same search result.
  cross_match              ops.cross_match with every source's hits on its own track blanked: the work ops.self_match
                           does (it drops them), and the six outputs must equal self_match's bit for bit
  cross_match_all_hits     nothing blanked: every source also finds the track it copies (a 303-row span to score)
  cross_match_pq[_all_hits]  the same two launches through ops.cross_match_pq against the library encoded at M = 64
                           (a quantiser trained on the first 65 536 rows; the codes decide the rows that are scored, not
                           the work)
--cross --tempo-ratios 1,15,31: ops.cross_match_tempo (csrc/crossmatch_tempo.hip) at grids of that many ratios against
dense ops.cross_match on the same tensors, alternating in one loop (medians of --reps).  The sources are the library's
rows taken along the slope of the grid ratio 266 (+4 %): every track as one source (as many rows as stay inside the
track), or with --tempo-source-rows N one source of N rows that runs on through the tracks from library row 0 (37 500:
an hour).  Their hits are the self-search's.  Also reports the workspace bytes of every launch and how many sources
find their track at ratio 266 over their whole length.
--tempo X [--tempo-step G]: ops.self_match_tempo (csrc/selfmatch_tempo.hip) over the ratio grid of
library.tempo_ratios(X, 256, G) (0.06 at step 1: 31 ratios) next to ops.self_match on the same library and hits,
alternating in one loop (medians of --reps).  Also reports the workspace bytes of both launches and what the sloped launch
makes of the planted copies (which run at ratio 256): the share whose partner it lists, the share it lists at the exact
offset and ratio 256, and the median of its span's rows over the dense launch's (a partner's best is its highest MEAN over
all ratios, so a cleaner part of a noisy copy, cut out by a neighbouring ratio, can outscore the whole span).  Expected
cost: about R dense passes plus the merge.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times))


def _cross(ops, rows, first, ids, per, reps):
    """The cross mode (see the top): sources = copies of the library's tracks, src_first = the track table."""
    from grafp_amd.ivfpq import IVFPQIndex
    n = rows.shape[0]
    q = rows.clone()
    own = torch.arange(n, device=rows.device) // per                       # the track of every row
    blanked = torch.where(torch.div(ids, per, rounding_mode="floor") == own[:, None], -1, ids)
    kw = dict(top=8, min_votes=4)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in
               zip(ops.cross_match(rows, first, q, first, blanked, **kw), ops.self_match(rows, first, ids, **kw)))
    res = {"cross_match_equals_self_match": bool(same),
           "cross_match_ms": _events(lambda: ops.cross_match(rows, first, q, first, blanked, **kw), reps) * 1e3,
           "cross_match_all_hits_ms": _events(lambda: ops.cross_match(rows, first, q, first, ids, **kw), reps) * 1e3}
    pq = IVFPQIndex(d=128, nlist=64, M=64, device=rows.device, niter=8, keep_raw=False)
    pq.train(rows[:65536])
    parts = [pq.encode(rows[lo:lo + 65536]) for lo in range(0, n, 65536)]
    lid, codes = torch.cat([p[0] for p in parts]).to(torch.int32), torch.cat([p[1] for p in parts])
    args = (lid, codes, pq.centroids, pq.codebooks, first, q, first)
    res["cross_match_pq_ms"] = _events(lambda: ops.cross_match_pq(*args, blanked, **kw), reps) * 1e3
    res["cross_match_pq_all_hits_ms"] = _events(lambda: ops.cross_match_pq(*args, ids, **kw), reps) * 1e3
    b_, d_ = (x.cpu().numpy() for x in ops.cross_match_pq(*args, ids, **kw)[:2])
    res["pq_sources_that_find_their_track_at_delta_0"] = int(((b_[:, 0] == np.arange(len(b_))) & (d_[:, 0] == 0)).sum())
    return {k: round(v, 3) if isinstance(v, float) else v for k, v in res.items()}


def _tempo(ops, rows, first, ids, per, reps, counts, source_rows):
    """The tempo mode (see the top)."""
    n, dev, num = rows.shape[0], rows.device, 266
    T = first.numel() - 1
    if source_rows:
        L = min(int(source_rows), (n - 1) * 256 // num)
        g = (torch.arange(L, device=dev, dtype=torch.int64) * num + 128) >> 8
        lens = np.array([L], np.int64)
    else:
        at = (torch.arange(per, device=dev, dtype=torch.int64) * num + 128) >> 8
        at = at[at < per]
        L = int(at.numel())
        g = (first[:-1, None] + at[None, :]).reshape(-1)
        lens = np.full(T, L, np.int64)
    q, hits = rows[g].contiguous(), ids[g].contiguous()
    src_first = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(dev)
    kw = dict(top=8, min_votes=4)
    grids = {}
    for R in counts:
        step = 1 if R == 1 else max(1, 30 // (R - 1))
        grids[R] = [num] if R == 1 else [256 + step * i for i in range(-(R // 2), R - R // 2)]
        assert num in grids[R] and len(grids[R]) == R, (R, grids[R])
    runs = {"cross_match_dense_ms": lambda: ops.cross_match(rows, first, q, src_first, hits, **kw)}
    for R, grid in grids.items():
        runs[f"cross_match_tempo_R{R}_ms"] = (lambda grid=grid: ops.cross_match_tempo(rows, first, q, src_first, hits,
                                                                                     grid, **kw))
    times = {name: [] for name in runs}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):                                                  # the launches alternate in one loop
        for name, fn in runs.items():
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    res = {"tempo_sources": int(len(lens)), "tempo_rows_per_source": L, "tempo_ratio": num}
    res.update({name: round(float(np.median(v)), 3) for name, v in times.items()})
    res["workspace_dense_bytes"] = ops.self_match_workspace_bytes(lens, ids.shape[1], 4)
    for R in grids:
        res[f"workspace_tempo_R{R}_bytes"] = ops.cross_match_tempo_workspace_bytes(lens, ids.shape[1], 4, R, 8)
        b_, _, lo_, m_, sc_, _, ra_ = (x.cpu().numpy() for x in runs[f"cross_match_tempo_R{R}_ms"]())
        whole = (ra_[:, 0] == num) & (lo_[:, 0] == 0) & (m_[:, 0] == L)
        res[f"tempo_R{R}_sources_found_whole_at_266"] = int(whole.sum())
        res[f"tempo_R{R}_best_rows_min"] = int(m_[:, 0].min())
    d = [x.cpu().numpy() for x in runs["cross_match_dense_ms"]()]
    res["dense_best_rows_max"] = int(d[3][:, 0].max())
    return res


def _self_tempo(ops, library, rows, first, ids, per, reps, tempo, step, planted):
    """The --tempo mode (see the top)."""
    grid = library.tempo_ratios(tempo, ops.IDENTIFY_TEMPO_DEN, 1 if step is None else step)
    kw = dict(top=8, min_votes=4)
    runs = {"self_match_dense_ms": lambda: ops.self_match(rows, first, ids, **kw),
            "self_match_tempo_ms": lambda: ops.self_match_tempo(rows, first, ids, grid, **kw)}
    times = {name: [] for name in runs}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):                                                  # the launches alternate in one loop
        for name, fn in runs.items():
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    res = {"tempo_ratios": int(len(grid)), "tempo_grid": [int(grid[0]), int(grid[-1])]}
    res.update({name: round(float(np.median(v)), 3) for name, v in times.items()})
    res["self_match_tempo_over_dense"] = round(res["self_match_tempo_ms"] / res["self_match_dense_ms"], 3)
    lens = np.full(first.numel() - 1, per, np.int64)
    res["workspace_dense_bytes"] = ops.self_match_workspace_bytes(lens, ids.shape[1], 4)
    res["workspace_tempo_bytes"] = ops.cross_match_tempo_workspace_bytes(lens, ids.shape[1], 4, len(grid), 8)
    b_, d_, _, m_, _, _, ra_ = (x.cpu().numpy() for x in runs["self_match_tempo_ms"]())
    db_, _, _, dm_, _, _ = (x.cpu().numpy() for x in runs["self_match_dense_ms"]())
    found, exact, share = 0, 0, []
    for src, dst, d in planted:
        for a, b, dd in ((src, dst, d), (dst, src, -d)):
            j = np.flatnonzero(b_[a] == b)
            found += j.size > 0
            exact += bool(j.size and d_[a, j[0]] == dd and ra_[a, j[0]] == 256)
            jd = np.flatnonzero(db_[a] == b)
            if j.size and jd.size:
                share.append(m_[a, j[0]] / dm_[a, jd[0]])
    res["tempo_planted_partner_found"] = round(found / max(1, 2 * len(planted)), 4)
    res["tempo_planted_exact_offset_at_256"] = round(exact / max(1, 2 * len(planted)), 4)
    res["tempo_planted_rows_over_dense_rows_median"] = round(float(np.median(share)), 4) if share else None
    return res


def main(argv=None):
    from grafp_amd import library, ops
    from grafp_amd.util import load_config
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=3300)
    ap.add_argument("--track-s", type=float, default=30.0)
    ap.add_argument("--copies", type=int, default=100)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cross", action="store_true", help="also time ops.cross_match and ops.cross_match_pq (M = 64)")
    ap.add_argument("--tempo-ratios", default=None,
                    help="with --cross: ratio counts, e.g. 1,15,31: time ops.cross_match_tempo against ops.cross_match")
    ap.add_argument("--tempo-source-rows", type=int, default=0,
                    help="with --tempo-ratios: one source of this many rows instead of every track as a source")
    ap.add_argument("--tempo", type=float, default=None,
                    help="also time ops.self_match_tempo over the ratios [1 - X, 1 + X] against ops.self_match")
    ap.add_argument("--tempo-step", type=int, default=None, help="with --tempo: the grid's spacing in 1/256 (default 1)")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    cfg = load_config()
    per = library.n_segments(int(args.track_s * cfg["fs"]), cfg)
    T = args.tracks
    n = T * per
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.randn((n, 128), generator=g, device=dev)
    rows /= rows.norm(dim=1, keepdim=True)
    first = torch.arange(T + 1, device=dev, dtype=torch.int64) * per
    rng = np.random.RandomState(1)
    pick = rng.permutation(T)[:2 * args.copies]
    planted = []
    for c in range(args.copies):
        src, dst = int(pick[2 * c]), int(pick[2 * c + 1])
        ln = int(rng.randint(40, per // 2))
        so, do = int(rng.randint(0, per - ln + 1)), int(rng.randint(0, per - ln + 1))
        noisy = rows[src * per + so:src * per + so + ln] + 0.4 / np.sqrt(128) * torch.randn(
            (ln, 128), generator=g, device=dev)
        rows[dst * per + do:dst * per + do + ln] = noisy / noisy.norm(dim=1, keepdim=True)
        planted.append((src, dst, do - so))

    index = ops.FlatL2Index(device=dev)
    index.add(rows)
    t_search = _events(lambda: index.search(rows, args.k), max(1, args.reps // 2))
    _, ids = index.search(rows, args.k)
    t_sm = _events(lambda: ops.self_match(rows, first, ids, top=8, min_votes=4), args.reps)
    b_, d_, _, _, sc, _ = (x.cpu().numpy() for x in ops.self_match(rows, first, ids, top=8, min_votes=4))
    hit = 0
    for src, dst, d in planted:
        hit += any(b_[src, j] == dst and d_[src, j] == d for j in range(8))
        hit += any(b_[dst, j] == src and d_[dst, j] == -d for j in range(8))
    planted_pairs = {(s, d) for s, d, _ in planted} | {(d, s) for s, d, _ in planted}
    stray = [float(sc[a, j]) for a in range(T) for j in range(8) if b_[a, j] >= 0 and (a, int(b_[a, j])) not in
             planted_pairs]
    out = {"rows": n, "tracks": T, "rows_per_track": per, "k": args.k, "copies": args.copies,
           "search_ms": round(t_search * 1e3, 3), "self_match_ms": round(t_sm * 1e3, 3),
           "self_match_over_search": round(t_sm / t_search, 4),
           "recall_exact_offset": round(hit / (2 * len(planted)), 4),
           "stray_pairs": len(stray), "max_stray_score": round(max(stray), 4) if stray else None}
    if args.tempo is not None:
        out.update(_self_tempo(ops, library, rows, first, ids, per, args.reps, args.tempo, args.tempo_step, planted))
    if args.cross:
        out.update(_cross(ops, rows, first, ids, per, args.reps))
        if args.tempo_ratios:
            out.update(_tempo(ops, rows, first, ids, per, args.reps, [int(v) for v in args.tempo_ratios.split(",")],
                              args.tempo_source_rows))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
