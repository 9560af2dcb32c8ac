"""Times ops.time_stretch (csrc/stretch.hip) with device events, next to ops.speed_change at the same shapes; prints one
line per case and one JSON line.

B = 256, 1 024 and 2 048 clips of 16 000 outputs (64 frames, 63 of them searched: 256 candidates x 512 products each),
at ratios drawn in [0.94, 1.06] (the training range), at the two ends 0.5 and 2, and at 1 (the copy).  Per case: the
median time, the time per searched frame of one clip's workgroup, and the correlation products per second against the
39.3 T fma/s of the vector units without packed-f32 instructions (256 CUs x 64 lanes x 2.4 GHz).  `--check` also compares
one batch against the float64 rule (tests/_stretch_ref.py): the shifts on the kernel's own path, and the output in units
of e32.
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

PEAK_FMA = 256 * 64 * 2.4e9
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


def bench(dev, reps):
    from grafp_amd import ops
    rows = []
    frames = ops.stretch_frames(T_OUT)
    for B in (256, 1024, 2048):
        pad, T_in = ops.stretch_pad(2.0), ops.stretch_input_len(T_OUT, 2.0)
        x = torch.rand((B, T_in), device=dev) * 2 - 1
        out = torch.empty((B, T_OUT), device=dev)
        g = torch.Generator(device=dev).manual_seed(B)
        cases = {"0.94-1.06": 0.94 + 0.12 * torch.rand(B, device=dev, generator=g),
                 "0.5": torch.full((B,), 0.5, device=dev), "2.0": torch.full((B,), 2.0, device=dev),
                 "1.0 (copy)": torch.ones(B, device=dev)}
        spad, s_in = ops.speed_pad(2.0), ops.speed_input_len(T_OUT, 2.0)
        for name, ratio in cases.items():
            med, lo, hi = _median_ms(lambda: ops.time_stretch(x, ratio, T_OUT, x_offset=pad, out=out), reps)
            speed, _, _ = _median_ms(lambda: ops.speed_change(x[:, :s_in], ratio, T_OUT, x_offset=spad, out=out), reps)
            fma = 0.0 if "copy" in name else float(B) * (frames - 1) * 256 * 512
            row = {"B": B, "ratios": name, "ms": med, "ms_min": lo, "ms_max": hi, "speed_change_ms": speed,
                   "us_per_frame": med * 1e3 / (frames - 1), "Tfma_per_s": fma / med / 1e9,
                   "fraction_of_fma_peak": fma / (med * 1e-3) / PEAK_FMA}
            print(f"B={B:5d} ratios {name:10s}: {med:8.4f} ms (min {lo:.4f} max {hi:.4f})  {row['us_per_frame']:6.2f} us per frame  "
                  f"{row['Tfma_per_s']:6.2f} Tfma/s ({100 * row['fraction_of_fma_peak']:.1f} % of 39.3)   speed_change {speed:.4f} ms")
            rows.append(row)
    return rows


def check(dev):
    from _stretch_ref import check_shifts, music_rows, stretch_f32, stretch_f64
    from grafp_amd import ops
    ratios = np.array([0.5, 0.7, 0.94, 0.97, 1.03, 1.06, 1.5, 2.0], dtype=np.float32)
    T = 4000
    pad, T_in = ops.stretch_pad(2.0), ops.stretch_input_len(T, 2.0)
    x = music_rows(T_in, range(20, 20 + len(ratios)))
    got, shifts = ops.time_stretch(torch.from_numpy(x).to(dev), torch.from_numpy(ratios).to(dev), T, x_offset=pad,
                                   return_shifts=True)
    got, shifts = got.double().cpu().numpy(), shifts.cpu().numpy()
    rows = []
    for b, r in enumerate(ratios):
        on_path = check_shifts(x[b], float(r), T, pad, shifts[b])              # raises if a shift is outside its bound
        own = stretch_f64(x[b], float(r), T, pad)
        r32 = stretch_f32(x[b], r, T, pad, shifts[b])
        e32, err = float(np.abs(r32 - on_path.out).max()), float(np.abs(got[b] - on_path.out).max())
        d32 = float(np.abs(got[b] - r32).max())
        same = int((shifts[b] == own.shifts).sum())
        print(f"rho={r:.2f}: shifts within their bounds, {same}/{shifts[b].size} equal to the rule's own path;  e32 {e32:.3e}  "
              f"kernel vs f64 {err:.3e} ({err / e32:.2f} e32)  kernel vs the f32 restatement {d32:.3e}")
        rows.append({"rho": float(r), "e32": e32, "err": err, "vs_f32": d32, "shifts_equal": same, "frames": int(shifts[b].size)})
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
