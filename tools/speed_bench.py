"""Times ops.speed_change (csrc/speed.hip) with device events; prints one line per case and one JSON line.

B = 256, 1 024 and 2 048 clips of 16 000 outputs, at ratios drawn in [0.94, 1.06] (the training range: 13 or 14 taps per
output) and at the two ends 0.5 (13 taps) and 2 (25 taps).  Per case: the median time, GB/s against the floor of one read
of the input span and one write of the output, and outputs x taps per second.  `--check` also compares one batch against
the float64 rule (tests/_speed_ref.py) and reports the kernel's error in units of e32.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_HBM = 8.0e12
T_OUT = 16000


def _median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def taps_per_output(rho):
    """Mean number of taps of the rule's sum at ratio rho: 2 * 6 / c + 1 samples wide, to within one."""
    return 2.0 * 6.0 / (0.99 * min(1.0, 1.0 / rho)) + 1.0


def bench(dev, reps):
    from grafp_amd import ops
    rows = []
    for B in (256, 1024, 2048):
        pad, T_in = ops.speed_pad(2.0), ops.speed_input_len(T_OUT, 2.0)
        x = torch.rand((B, T_in), device=dev) * 2 - 1
        out = torch.empty((B, T_OUT), device=dev)
        g = torch.Generator(device=dev).manual_seed(B)
        cases = {"0.94-1.06": 0.94 + 0.12 * torch.rand(B, device=dev, generator=g),
                 "0.5": torch.full((B,), 0.5, device=dev), "2.0": torch.full((B,), 2.0, device=dev),
                 "1.0 (copy)": torch.ones(B, device=dev)}
        for name, ratio in cases.items():
            med, lo, hi = _median_ms(lambda: ops.speed_change(x, ratio, T_OUT, x_offset=pad, out=out), reps)
            r = ratio.double().cpu().numpy()
            floor_bytes = 4.0 * (float(np.sum(T_OUT * r)) + B * T_OUT)          # the span read once, the output written once
            taps = float(np.sum([taps_per_output(v) for v in r])) * T_OUT if "copy" not in name else 0.0
            row = {"B": B, "ratios": name, "ms": med, "ms_min": lo, "ms_max": hi, "floor_GBps": floor_bytes / med / 1e6,
                   "fraction_of_hbm_peak": floor_bytes / (med * 1e-3) / PEAK_HBM, "Gtaps_per_s": taps / med / 1e6}
            print(f"B={B:5d} ratios {name:10s}: {med:8.4f} ms (min {lo:.4f} max {hi:.4f})  {row['floor_GBps']:8.1f} GB/s of "
                  f"read+write floor ({100 * row['fraction_of_hbm_peak']:.1f} % of 8 TB/s)  {row['Gtaps_per_s']:8.1f} Gtap/s")
            rows.append(row)
    return rows


def check(dev):
    from _speed_ref import batch_refs, uniform_rows
    from grafp_amd import ops
    ratios = np.array([0.5, 0.7, 0.94, 0.97, 1.03, 1.06, 1.5, 2.0], dtype=np.float32)
    pad, T_in = ops.speed_pad(2.0), ops.speed_input_len(4000, 2.0)
    x = uniform_rows(len(ratios), T_in, 5)
    got = ops.speed_change(torch.from_numpy(x).to(dev), torch.from_numpy(ratios).to(dev), 4000, x_offset=pad)
    r64, r32 = batch_refs(x, ratios, 4000, pad)
    got = got.double().cpu().numpy()
    rows = []
    for b, r in enumerate(ratios):
        e32, err = float(np.abs(r32[b] - r64[b]).max()), float(np.abs(got[b] - r64[b]).max())
        d32 = float(np.abs(got[b] - r32[b]).max())
        print(f"rho={r:.2f}: e32 {e32:.3e}  kernel vs f64 {err:.3e} ({err / e32:.2f} e32)  kernel vs the f32 restatement {d32:.3e}")
        rows.append({"rho": float(r), "e32": e32, "err": err, "vs_f32": d32})
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": bench(dev, args.reps)}
    if args.check:
        res["check"] = check(dev)
    print(json.dumps(res))
