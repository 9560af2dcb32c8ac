"""Measurements of track-aware identification (ops.identify, csrc/identify.hip); prints one JSON line.

A library of --tracks tracks x --track-s seconds (default 3 300 x 30 s: 303 segments each, about 1 M rows of random unit
fingerprints), --queries items of --qlen segments (default 4 096 x 31) planted at random in-track alignments with noise,
one batched search at k = --k (default 20), then:
  search      ops.FlatL2Index.search of every query row (bf16 pre-filter, exact)
  identify    ops.identify of all items in one launch (top 5)
  seq_rerank  ops.seq_rerank of the same items and hits (top 10), the row-level rerank of eval.py, as the comparison
Kernel times from events (median of --reps); `rocprofv3 --kernel-trace --stats -- python tools/identify_bench.py` gives
the per-kernel figures.
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
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--qlen", type=int, default=31)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    cfg = load_config()
    per = library.n_segments(int(args.track_s * cfg["fs"]), cfg)
    T, ql, nq = args.tracks, args.qlen, args.queries
    n = T * per
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.randn((n, 128), generator=g, device=dev)
    rows /= rows.norm(dim=1, keepdim=True)
    first = torch.arange(T + 1, device=dev, dtype=torch.int64) * per
    rng = np.random.RandomState(1)
    t = rng.randint(0, T, size=nq)
    a = t * per + rng.randint(0, per - ql + 1, size=nq)
    src = torch.from_numpy((a[:, None] + np.arange(ql)[None]).reshape(-1)).to(dev)
    q = rows[src] + 0.5 / np.sqrt(128) * torch.randn((nq * ql, 128), generator=g, device=dev)
    q /= q.norm(dim=1, keepdim=True)
    item_row = torch.arange(nq, device=dev, dtype=torch.int64) * ql
    item_len = torch.full((nq,), ql, device=dev, dtype=torch.int32)

    index = ops.FlatL2Index(device=dev)
    index.add(rows)
    t_search = _events(lambda: index.search(q, args.k), max(1, args.reps // 4))
    _, ids = index.search(q, args.k)
    t_id = _events(lambda: ops.identify(rows, first, q, ids, item_row, item_len, top=5, max_len=ql), args.reps)
    t_rr = _events(lambda: ops.seq_rerank(rows, q, ids, item_row, item_len, top=10, max_len=ql), args.reps)
    tr, off, sc, vo = ops.identify(rows, first, q, ids, item_row, item_len, top=5, max_len=ql)
    want_off = torch.from_numpy(a - t * per).to(dev)
    hit = (tr[:, 0].long() == torch.from_numpy(t).to(dev)) & (off[:, 0].long() == want_off)
    out = {"rows": n, "tracks": T, "queries": nq, "qlen": ql, "k": args.k,
           "search_ms": round(t_search * 1e3, 3), "identify_ms": round(t_id * 1e3, 3),
           "seq_rerank_ms": round(t_rr * 1e3, 3), "identify_over_seq_rerank": round(t_id / t_rr, 3),
           "identify_top1_correct": round(float(hit.float().mean()), 4),
           "mean_votes_top1": round(float(vo[:, 0].float().mean()), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
