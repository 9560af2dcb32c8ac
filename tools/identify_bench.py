"""Measurements of track-aware identification (ops.identify, csrc/identify.hip); prints one JSON line.

A library of --tracks tracks x --track-s seconds (default 3 300 x 30 s: 303 segments each, about 1 M rows of random unit
fingerprints), --queries items of --qlen segments (default 4 096 x 31) planted at random in-track alignments with noise,
one batched search at k = --k (default 20), then:
  search      ops.FlatL2Index.search of every query row (bf16 pre-filter, exact)
  identify    ops.identify of all items in one launch (top 5)
  seq_rerank  ops.seq_rerank of the same items and hits (top 10), the row-level rerank of eval.py, as the comparison
With --index ivfpq the library is held as IVF-PQ codes (ivfpq.IVFPQIndex, keep_raw=False: --nlist, --pq-m, --nprobe) and
the two stages of a query against a compact library are reported separately:
  ivfpq_search   IVFPQIndex.search of every query row
  identify_pq    ops.identify_pq of all items on the codes, next to ops.identify of the same items and hits on the
                 decoded rows (index.reconstruct()), and their ratio
With --row-stride D the flat library keeps every D-th row of each track (FingerprintLibrary.thin) and the same dense
items are identified against it:
  search         ops.FlatL2Index.search of every query row over the kept rows
  identify_thin  ops.identify_thin of all items in one launch (top 5), next to ops.identify of the same items on the
                 dense library, and the library's bytes per original row
With --tempo-ratios R1,R2,... the items are the library's own rows along the slope of ratio --tempo-num / 256 (default
266: 4 % fast) and their hits are made, not searched: the planted row, its four neighbours and random rows (the search is
the same with and without a tempo, and at 4 096 items of 94 rows it would take the run).  For every R:
  identify_tempo  ops.identify_tempo of all items over the R ratios 256 - 2 * (R // 2) ... in steps of 2 (plus 266 if it
                  is not among them), next to ops.identify of the same items and hits, calls alternating, and the top-1
                  hit rate of both
With --tempo-items (next to --tempo-ratios' planted items; the ratio counts given are not used) the same items are
identified over the three ratios num - 4, num, num + 4 in two ways, calls alternating:
  identify_tempo        ops.identify_tempo with those three ratios
  identify_tempo_items  ops.identify_tempo_items over the grid num - 12 ... num + 12 in steps of 4 (7 ratios), every item
                        with the window lo = 2, cnt = 3: the same workgroups' work behind a work table (host time of the
                        table and its upload included), medians with min and max, and whether the outputs are bit-equal
With --query-stride Q only every Q-th row of every item is kept (rows 0, Q, 2 Q, ... of its --qlen: ceil(qlen / Q) rows):
  search           ops.FlatL2Index.search of the kept query rows, next to the search of all of them
  identify_stride  ops.identify_stride of the kept items in one launch (top 5), next to ops.identify of the same items
                   with Q times the rows, and the top-1 hit rate of both
With --index half the library is held as bf16 rows (B = ops.rows_to_bf16(rows)) next to the flat library over their f32
values U, in the same process, calls alternating:
  search_half    ops.HalfL2Index.search of every query row, next to ops.FlatL2Index.search over U
  identify_half  ops.identify_half of all items on B, next to ops.identify of the same items and hits on U, their ratio,
                 whether the two are bit-equal, and the bytes per row of both forms
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


def _ivfpq(args, dev, rows, first, q, item_row, item_len, true_track, true_off):
    from grafp_amd import ops
    from grafp_amd.ivfpq import IVFPQIndex
    ql = args.qlen
    index = IVFPQIndex(nlist=args.nlist, M=args.pq_m, device=dev, keep_raw=False)
    index.train(rows)
    index.add(rows)
    index.nprobe = args.nprobe
    list_id, codes = index.codes_by_row()
    quant = index.quantiser()
    cent, books = quant["centroids"], quant["codebooks"]
    t_search = _events(lambda: index.search(q, args.k), max(1, args.reps // 4))
    _, ids = index.search(q, args.k)
    run_pq = lambda: ops.identify_pq(list_id, codes, cent, books, first, q, ids, item_row, item_len, top=5, max_len=ql)
    t_pq = _events(run_pq, args.reps)
    dec = index.reconstruct()
    run_dec = lambda: ops.identify(dec, first, q, ids, item_row, item_len, top=5, max_len=ql)
    t_dec = _events(run_dec, args.reps)
    got, want = run_pq(), run_dec()
    same = all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want))
    tr, off = got[0], got[1]
    hit = (tr[:, 0].long() == torch.from_numpy(true_track).to(dev)) & \
          (off[:, 0].long() == torch.from_numpy(true_off).to(dev))
    return {"index": "ivfpq", "rows": int(rows.shape[0]), "tracks": int(first.numel() - 1), "queries": args.queries,
            "qlen": ql, "k": args.k, "nlist": args.nlist, "M": args.pq_m, "nprobe": args.nprobe,
            "ivfpq_search_ms": round(t_search * 1e3, 3), "identify_pq_ms": round(t_pq * 1e3, 3),
            "identify_decoded_ms": round(t_dec * 1e3, 3), "identify_pq_over_identify": round(t_pq / t_dec, 3),
            "bit_equal_to_identify_on_decoded_rows": bool(same),
            "identify_top1_correct": round(float(hit.float().mean()), 4)}


def _half(args, dev, rows, first, q, item_row, item_len, true_track, true_off):
    from grafp_amd import ops
    ql = args.qlen
    b = ops.rows_to_bf16(rows)
    u = b.float()
    half, flat = ops.HalfL2Index(device=dev), ops.FlatL2Index(device=dev)
    half.add(b)
    flat.add(u)
    _, ids = half.search(q, args.k)
    same_ids = torch.equal(ids, flat.search(q, args.k)[1])
    run_h = lambda: ops.identify_half(b, first, q, ids, item_row, item_len, top=5, max_len=ql)
    run_f = lambda: ops.identify(u, first, q, ids, item_row, item_len, top=5, max_len=ql)
    pairs = {"search": (lambda: flat.search(q, args.k), lambda: half.search(q, args.k), max(1, args.reps // 4)),
             "identify": (run_f, run_h, args.reps)}
    times = {}
    for name, (f_call, h_call, reps) in pairs.items():
        for _ in range(2):
            f_call(), h_call()
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        tf, th = [], []
        for _ in range(reps):                               # alternating, one synchronise per pair
            e[0].record()
            f_call()
            e[1].record()
            h_call()
            e[2].record()
            torch.cuda.synchronize()
            tf.append(e[0].elapsed_time(e[1]))
            th.append(e[1].elapsed_time(e[2]))
        times[name] = (float(np.median(tf)), float(np.median(th)))
    got, want = run_h(), run_f()
    same = all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want))
    hit = (got[0][:, 0].long() == torch.from_numpy(true_track).to(dev)) & \
          (got[1][:, 0].long() == torch.from_numpy(true_off).to(dev))
    n = int(rows.shape[0])
    flat_bytes = sum(t.numel() * t.element_size() for t in flat.held_tensors())
    return {"index": "half", "rows": n, "tracks": int(first.numel() - 1), "queries": args.queries, "qlen": ql,
            "k": args.k, "search_flat_ms": round(times["search"][0], 3), "search_half_ms": round(times["search"][1], 3),
            "identify_flat_ms": round(times["identify"][0], 3), "identify_half_ms": round(times["identify"][1], 3),
            "identify_half_over_identify": round(times["identify"][1] / times["identify"][0], 3),
            "search_ids_equal": bool(same_ids), "bit_equal_to_identify_on_widened_rows": bool(same),
            "bytes_per_row_flat": round(flat_bytes / n, 1), "bytes_per_row_half": round(half.nbytes / n, 1),
            "identify_top1_correct": round(float(hit.float().mean()), 4)}


def _thin(args, dev, cfg, rows, first, q, item_row, item_len, true_track, true_off):
    from grafp_amd import library, ops
    ql, D = args.qlen, args.row_stride
    dense = library.FingerprintLibrary(None, cfg, rows, first.cpu().numpy(), precision="f32", device=dev)
    thin = dense.thin(D)
    trows, tfirst = thin.rows(), torch.from_numpy(thin.first).to(dev)
    t_search = _events(lambda: thin.index.search(q, args.k), max(1, args.reps // 4))
    _, ids = thin.index.search(q, args.k)
    run = lambda: ops.identify_thin(trows, tfirst, q, ids, item_row, item_len, D, top=5, max_len=ql)
    t_thin = _events(run, args.reps)
    tr, off, _, vo = run()
    hit = (tr[:, 0].long() == torch.from_numpy(true_track).to(dev)) & \
          (off[:, 0].long() == torch.from_numpy(true_off).to(dev))
    nbytes = thin.nbytes
    _, dids = dense.index.search(q, args.k)
    t_dense = _events(lambda: ops.identify(rows, first, q, dids, item_row, item_len, top=5, max_len=ql), args.reps)
    return {"row_stride": D, "rows": int(rows.shape[0]), "kept_rows": thin.n_rows, "tracks": thin.n_tracks,
            "queries": args.queries, "qlen": ql, "k": args.k, "search_ms": round(t_search * 1e3, 3),
            "identify_thin_ms": round(t_thin * 1e3, 3), "identify_dense_ms": round(t_dense * 1e3, 3),
            "bytes_per_original_row": round(nbytes / rows.shape[0], 1),
            "identify_top1_correct": round(float(hit.float().mean()), 4),
            "mean_votes_top1": round(float(vo[:, 0].float().mean()), 2)}


def _stride(args, dev, rows, first, q, item_row, item_len, true_track, true_off):
    from grafp_amd import ops
    ql, Q, nq = args.qlen, args.query_stride, args.queries
    kl = -(-ql // Q)
    keep = (np.arange(nq)[:, None] * ql + np.arange(kl)[None] * Q).reshape(-1)
    qk = q[torch.from_numpy(keep).to(dev)].contiguous()
    krow = torch.arange(nq, device=dev, dtype=torch.int64) * kl
    klen = torch.full((nq,), kl, device=dev, dtype=torch.int32)
    index = ops.FlatL2Index(device=dev)
    index.add(rows)
    t_search_dense = _events(lambda: index.search(q, args.k), max(1, args.reps // 4))
    t_search = _events(lambda: index.search(qk, args.k), max(1, args.reps // 4))
    _, ids = index.search(q, args.k)
    _, kids = index.search(qk, args.k)
    dense = lambda: ops.identify(rows, first, q, ids, item_row, item_len, top=5, max_len=ql)
    strided = lambda: ops.identify_stride(rows, first, qk, kids, krow, klen, Q, top=5, max_len=kl)
    t_dense, t_stride = _events(dense, args.reps), _events(strided, args.reps)
    want_t, want_o = torch.from_numpy(true_track).to(dev), torch.from_numpy(true_off).to(dev)
    hit = lambda out: round(float(((out[0][:, 0].long() == want_t) & (out[1][:, 0].long() == want_o)).float().mean()), 4)
    return {"query_stride": Q, "rows": int(rows.shape[0]), "tracks": int(first.numel() - 1), "queries": nq, "qlen": ql,
            "kept_qlen": kl, "k": args.k, "search_ms": round(t_search * 1e3, 3),
            "search_dense_ms": round(t_search_dense * 1e3, 3), "identify_stride_ms": round(t_stride * 1e3, 3),
            "identify_dense_ms": round(t_dense * 1e3, 3), "stride_over_dense": round(t_stride / t_dense, 3),
            "identify_stride_top1_correct": hit(strided()), "identify_dense_top1_correct": hit(dense())}


def _tempo(args, dev, rows, first, per):
    from grafp_amd import ops
    T, ql, nq, k, num = args.tracks, args.qlen, args.queries, args.k, args.tempo_num
    n = rows.shape[0]
    rng = np.random.RandomState(2)
    at = (np.arange(ql) * num + 128) >> 8
    t = rng.randint(0, T, size=nq)
    p0 = rng.randint(0, per - int(at[-1]), size=nq)
    src = ((t * per + p0)[:, None] + at[None]).reshape(-1)
    q = rows[torch.from_numpy(src).to(dev)].contiguous()
    ids = rng.randint(0, n, size=(nq * ql, k)).astype(np.int64)
    for c, d in enumerate((0, 1, -1, 2, -2)):
        ids[:, c] = np.clip(src + d, 0, n - 1)
    ids = torch.from_numpy(ids).to(dev)
    item_row = torch.arange(nq, device=dev, dtype=torch.int64) * ql
    item_len = torch.full((nq,), ql, device=dev, dtype=torch.int32)
    want_t, want_o = torch.from_numpy(t).to(dev), torch.from_numpy(p0).to(dev)
    dense = lambda: ops.identify(rows, first, q, ids, item_row, item_len, top=5, max_len=ql)
    out = {"rows": int(n), "tracks": T, "queries": nq, "qlen": ql, "k": k, "planted_num": num, "by_ratios": []}
    if args.tempo_items:
        three, grid = [num - 4, num, num + 4], list(range(num - 12, num + 13, 4))
        lo, cnt = np.full(nq, 2, np.int64), np.full(nq, 3, np.int64)
        whole = lambda: ops.identify_tempo(rows, first, q, ids, item_row, item_len, three, top=5, max_len=ql)
        items = lambda: ops.identify_tempo_items(rows, first, q, ids, item_row, item_len, grid, lo, cnt, top=5,
                                                 max_len=ql)
        for _ in range(3):
            whole(), items()
        torch.cuda.synchronize()
        tw, ti = [], []
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        for _ in range(args.reps):                          # alternating, one synchronise per pair
            a.record()
            whole()
            b.record()
            items()
            c.record()
            torch.cuda.synchronize()
            tw.append(a.elapsed_time(b))
            ti.append(b.elapsed_time(c))
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(whole(), items()))
        del out["by_ratios"]
        out.update({"ratios": three, "identify_tempo_ms": round(float(np.median(tw)), 4),
                    "identify_tempo_ms_min_max": [round(min(tw), 4), round(max(tw), 4)],
                    "identify_tempo_items_ms": round(float(np.median(ti)), 4),
                    "identify_tempo_items_ms_min_max": [round(min(ti), 4), round(max(ti), 4)],
                    "items_over_whole": round(float(np.median(ti) / np.median(tw)), 3), "bit_equal": bool(same)})
        return out
    for R in args.tempo_ratios:
        nums = sorted(set([256 + 2 * (i - R // 2) for i in range(R)] + ([num] if R > 1 else [])))
        sloped = lambda: ops.identify_tempo(rows, first, q, ids, item_row, item_len, nums, top=5, max_len=ql)
        for _ in range(3):
            dense(), sloped()
        torch.cuda.synchronize()
        td, ts = [], []
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        for _ in range(args.reps):                          # alternating, one synchronise per pair
            a.record()
            dense()
            b.record()
            sloped()
            c.record()
            torch.cuda.synchronize()
            td.append(a.elapsed_time(b))
            ts.append(b.elapsed_time(c))
        tr, off, sc, _, ra = sloped()
        dt, do, ds, _ = dense()
        hit = (tr[:, 0].long() == want_t) & (off[:, 0].long() == want_o)
        dhit = dt[:, 0].long() == want_t
        out["by_ratios"].append({"R": len(nums), "identify_tempo_ms": round(float(np.median(ts)), 4),
                                 "identify_ms": round(float(np.median(td)), 4),
                                 "tempo_over_dense": round(float(np.median(ts) / np.median(td)), 3),
                                 "tempo_ms_min_max": [round(min(ts), 4), round(max(ts), 4)],
                                 "dense_ms_min_max": [round(min(td), 4), round(max(td), 4)],
                                 "tempo_top1_track_and_offset": round(float(hit.float().mean()), 4),
                                 "tempo_top1_score": round(float(sc[:, 0].mean()), 4),
                                 "dense_top1_track": round(float(dhit.float().mean()), 4),
                                 "dense_top1_score": round(float(ds[:, 0].mean()), 4)})
    return out


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
    ap.add_argument("--index", choices=("flat", "ivfpq", "half"), default="flat")
    ap.add_argument("--nlist", type=int, default=64)
    ap.add_argument("--pq-m", type=int, default=64)
    ap.add_argument("--nprobe", type=int, default=20)
    ap.add_argument("--row-stride", type=int, default=None, help="flat: keep every D-th row of each track")
    ap.add_argument("--query-stride", type=int, default=None, help="flat: keep every Q-th row of each item")
    ap.add_argument("--tempo-ratios", type=lambda v: [int(x) for x in v.split(",")], default=None,
                    help="ratio counts to time ops.identify_tempo at, e.g. 1,15,31")
    ap.add_argument("--tempo-items", action="store_true",
                    help="tempo: ops.identify_tempo at 3 ratios against ops.identify_tempo_items with windows of 3")
    ap.add_argument("--tempo-num", type=int, default=266, help="tempo: the ratio the items are planted at (num / 256)")
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
    if args.tempo_ratios is not None or args.tempo_items:
        print(json.dumps(_tempo(args, dev, rows, first, per)))
        return
    rng = np.random.RandomState(1)
    t = rng.randint(0, T, size=nq)
    a = t * per + rng.randint(0, per - ql + 1, size=nq)
    src = torch.from_numpy((a[:, None] + np.arange(ql)[None]).reshape(-1)).to(dev)
    q = rows[src] + 0.5 / np.sqrt(128) * torch.randn((nq * ql, 128), generator=g, device=dev)
    q /= q.norm(dim=1, keepdim=True)
    item_row = torch.arange(nq, device=dev, dtype=torch.int64) * ql
    item_len = torch.full((nq,), ql, device=dev, dtype=torch.int32)

    if args.index == "ivfpq":
        print(json.dumps(_ivfpq(args, dev, rows, first, q, item_row, item_len, t, a - t * per)))
        return
    if args.index == "half":
        print(json.dumps(_half(args, dev, rows, first, q, item_row, item_len, t, a - t * per)))
        return
    if args.row_stride is not None:
        print(json.dumps(_thin(args, dev, cfg, rows, first, q, item_row, item_len, t, a - t * per)))
        return
    if args.query_stride is not None:
        print(json.dumps(_stride(args, dev, rows, first, q, item_row, item_len, t, a - t * per)))
        return
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
