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
    if args.cross:
        out.update(_cross(ops, rows, first, ids, per, args.reps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
