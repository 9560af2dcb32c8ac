"""Measurements of shared-audio detection inside a library (ops.self_match, csrc/selfmatch.hip); prints one JSON line.

A library of --tracks tracks x --track-s seconds (default 3 300 x 30 s: 303 segments each, about 1 M rows of random unit
fingerprints) with --copies planted copies (default 100): a noisy sub-range of one track written into another at a known
offset.  Then:
  search      ops.FlatL2Index.search of every library row against the library at k = --k (default 32), the self-search
  self_match  ops.self_match of all tracks in one launch (top 8, min_votes 4)
  recall      planted pairs found in both directions with the exact offset
Times from events (median of --reps); `rocprofv3 --kernel-trace --stats -- python tools/selfmatch_bench.py` gives the
per-kernel figures.  Target: self_match <= 0.25 x search.
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


def main(argv=None):
    from grafp_amd import library, ops
    from grafp_amd.util import load_config
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=3300)
    ap.add_argument("--track-s", type=float, default=30.0)
    ap.add_argument("--copies", type=int, default=100)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
