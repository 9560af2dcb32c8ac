"""tools/search_bench.py [--n ROWS] [--pre|--f32|--half] [NQ ...]: latency and throughput of ops.search_l2 per batch size on a
random unit-norm database (planted neighbours at sigma 0.05: top-1 must be 1.000).  --pre (default) = the bf16
pre-filter path (grafp_knn_search_l2_pre), --f32 = the all-f32 path.  --half = the half form (grafp_knn_search_l2_half:
the database held as bf16 rows only) next to the pre-filter path over the f32 values of the same rows, in the same process,
calls alternating, with the bytes of both and whether the results are bit-equal.  With GRAFP_HIP_LIB pointing at the measurement
build the plan knobs of csrc/tuning.h (GRAFP_SEARCH_NQS) can be swept from the environment."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grafp_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--f32", action="store_true")
    ap.add_argument("--half", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("nq", nargs="*", type=int)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2)
    db = torch.nn.functional.normalize(torch.randn(a.n, 128, generator=gen, device=dev), dim=1)
    rows = torch.randint(0, a.n, (4096,), generator=gen, device=dev)
    q = torch.nn.functional.normalize(db[rows] + 0.05 * torch.randn(4096, 128, generator=gen, device=dev), dim=1)
    if a.half:
        return half(a, db, q, rows)
    sq = ops.row_sqnorm(db)
    dbh = None if a.f32 else ops.rows_to_bf16(db)
    print(f"# {a.n} x 128, k = {a.k}, {'all-f32 path' if a.f32 else 'bf16 pre-filter + exact rescoring'}")
    for nq in a.nq or [1, 8, 41, 128, 512, 1024, 4096]:
        ops.search_l2(db, sq, q[:nq], a.k, db_bf16=dbh)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            D, I = ops.search_l2(db, sq, q[:nq], a.k, db_bf16=dbh)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.reps
        top1 = (I[:, 0] == rows[:nq]).float().mean().item()
        print(f"nq={nq:5d}  {dt * 1e3:8.3f} ms  {nq / dt:10.0f} QPS  top1 {top1:.3f}")


def half(a, db, q, rows):
    """The flat pre-filter path over U and the half path over B = rows_to_bf16(db), U = B.float(): per batch size the
    median of --reps alternating calls of each (device events), top-1 of the half path and whether the two agree bit for bit."""
    b = ops.rows_to_bf16(db)
    u = b.float()
    del db
    sq_u, sq_b = ops.row_sqnorm(u), ops.row_sqnorm_half(b)
    flat_bytes = u.numel() * 4 + b.numel() * 2 + sq_u.numel() * 4
    half_bytes = b.numel() * 2 + sq_b.numel() * 4
    print(f"# {a.n} x 128, k = {a.k}: flat (f32 rows + bf16 copy + norms) {flat_bytes} bytes, {flat_bytes / a.n:.0f} a row; "
          f"half (bf16 rows + norms) {half_bytes} bytes, {half_bytes / a.n:.0f} a row; norms equal: {torch.equal(sq_u, sq_b)}")
    flat_call = lambda nq: ops.search_l2(u, sq_u, q[:nq], a.k, db_bf16=b)
    half_call = lambda nq: ops.search_l2_half(b, sq_b, q[:nq], a.k)
    for nq in a.nq or [1, 41, 4096]:
        for _ in range(3):
            flat_call(nq), half_call(nq)
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        tf, th = [], []
        for _ in range(a.reps):
            e[0].record()
            Df, If = flat_call(nq)
            e[1].record()
            Dh, Ih = half_call(nq)
            e[2].record()
            torch.cuda.synchronize()
            tf.append(e[0].elapsed_time(e[1]))
            th.append(e[1].elapsed_time(e[2]))
        tf, th = sorted(tf), sorted(th)
        same = torch.equal(If, Ih) and torch.equal(Df.view(torch.int32), Dh.view(torch.int32))
        top1 = (Ih[:, 0] == rows[:nq]).float().mean().item()
        print(f"nq={nq:5d}  flat {tf[len(tf) // 2]:8.3f} ms [{tf[0]:.3f}, {tf[-1]:.3f}]  half {th[len(th) // 2]:8.3f} ms "
              f"[{th[0]:.3f}, {th[-1]:.3f}]  half/flat {th[len(th) // 2] / tf[len(tf) // 2]:.3f}  bit-equal {same}  "
              f"top1 {top1:.3f}")


if __name__ == "__main__":
    main()
