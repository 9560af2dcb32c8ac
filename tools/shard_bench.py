"""What sharding a fingerprint library costs on ONE device (grafp_amd/sharded.py, csrc/merge_lists.hip).

tools/identify_bench.py's library (unit random rows, --tracks tracks of --track-s seconds) and --queries items of --qlen
rows planted in it with noise.  Timed in one process, alternating, medians of --reps after 3 warm-up rounds, device
events around each call (a call ends in its own read-back, so the events see all of it):
  plain     FingerprintLibrary: _search_rows + _identify_items (search, one ops.identify launch, read-back, dicts)
  shards_1  the same on ShardedFingerprintLibrary.split(lib, 1): one shard's launches, the two merges
  shards_N  the same on split(lib, --shards), all shards on the one device: N launch sequences one after the other
  merge     ops.merge_track_lists alone on the N shards' lists of these items (--merge-launches launches per event pair)
and the three results are compared (they must be equal).  One shard per device is what sharding is for; this box times
what the extra launches and the merge cost where nothing runs side by side.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    from grafp_amd import library, ops
    from grafp_amd.sharded import ShardedFingerprintLibrary
    from grafp_amd.util import load_config
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=3300)
    ap.add_argument("--track-s", type=float, default=30.0)
    ap.add_argument("--queries", type=int, default=41)
    ap.add_argument("--qlen", type=int, default=94)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--shards", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--merge-launches", type=int, default=50)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    cfg = load_config()
    per = library.n_segments(int(args.track_s * cfg["fs"]), cfg)
    T, ql, nq = args.tracks, args.qlen, args.queries
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.randn((T * per, 128), generator=g, device=dev)
    rows /= rows.norm(dim=1, keepdim=True)
    first = np.arange(T + 1, dtype=np.int64) * per
    rng = np.random.RandomState(1)
    t = rng.randint(0, T, size=nq)
    a = t * per + rng.randint(0, per - ql + 1, size=nq)
    src = torch.from_numpy((a[:, None] + np.arange(ql)[None]).reshape(-1)).to(dev)
    q = rows[src] + 0.5 / np.sqrt(128) * torch.randn((nq * ql, 128), generator=g, device=dev)
    q /= q.norm(dim=1, keepdim=True)
    item_row = np.arange(nq, dtype=np.int64) * ql
    item_len = np.full(nq, ql, np.int32)

    plain = library.FingerprintLibrary(None, cfg, rows, first, precision="f32", device=dev)
    libs = {"plain": plain, "shards_1": ShardedFingerprintLibrary.split(plain, 1),
            f"shards_{args.shards}": ShardedFingerprintLibrary.split(plain, args.shards)}
    run = lambda lib: lib._identify_items(q, lib._search_rows(q, args.k), item_row, item_len, 5, None)
    results = {name: run(lib) for name, lib in libs.items()}
    for _ in range(3):
        for lib in libs.values():
            run(lib)
    torch.cuda.synchronize()
    times = {name: [] for name in libs}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(libs) + 1)]
    for _ in range(args.reps):
        ev[0].record()
        for j, lib in enumerate(libs.values()):
            run(lib)
            ev[j + 1].record()
        torch.cuda.synchronize()
        for j, name in enumerate(libs):
            times[name].append(ev[j].elapsed_time(ev[j + 1]))

    # the merge alone, on the lists these items give on the N shards
    sh = libs[f"shards_{args.shards}"]
    ids = sh._search_rows(q, args.k)
    live = sh._live()
    outs = [part._identify_lists(q, ids - int(sh.rb[s]), item_row, item_len, 5, None, ql) for s, part in live]
    track, score = torch.stack([o[0] for o in outs]), torch.stack([o[2] for o in outs])
    payload = torch.stack([torch.stack([o[j] for o in outs]) for j in (1, 3)])
    bases, pad = [int(sh.tb[s]) for s, _ in live], [-2 ** 31, 0]
    merge = lambda: ops.merge_track_lists(track, score, payload, bases, pad)
    for _ in range(3):
        merge()
    torch.cuda.synchronize()
    tm = []
    a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.reps):
        a_.record()
        for _ in range(args.merge_launches):
            merge()
        b_.record()
        torch.cuda.synchronize()
        tm.append(a_.elapsed_time(b_) / args.merge_launches)

    hit = float(np.mean([bool(r) and r[0]["track"] == int(tt) and r[0]["offset"] == int(aa - tt * per)
                         for r, tt, aa in zip(results["plain"], t, a)]))
    out = {"rows": int(rows.shape[0]), "tracks": T, "queries": nq, "qlen": ql, "k": args.k, "reps": args.reps,
           **{f"{name}_ms": round(float(np.median(v)), 4) for name, v in times.items()},
           **{f"{name}_ms_min_max": [round(min(v), 4), round(max(v), 4)] for name, v in times.items()},
           "merge_track_lists_ms": round(float(np.median(tm)), 5),
           "merge_shape_S_items_top_P": [len(live), nq, 5, 2],
           "rows_per_shard": [part.n_rows for part in sh.shards],
           "sharded_equal_to_plain": all(results[name] == results["plain"] for name in libs),
           "identify_top1_correct": round(hit, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
