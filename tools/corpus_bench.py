"""Measurements of the device-resident corpus (grafp_amd/data.py, csrc/corpus.hip); prints one JSON line.

  resample    256 tracks x 30 s, 44.1 -> 16 kHz, one launch: time, TFLOP/s (2*K flop per output), fraction of the f32
              vector peak (157.3 TFLOP/s)
  draw        draw_pairs at 1024 pairs: time and HBM rate on the algorithmic bytes (window read once + two views written)
  load        DeviceAudioCorpus over 44.1 kHz stereo 16-bit .wav files: decode / upload / resample / quantile seconds
  step        Trainer.step_graph at --batch pairs (bf16) fed by corpus.batches vs by synthetic_batch, and the peak device
              memory with the corpus resident
Kernel times from events here; `rocprofv3 --kernel-trace --stats -- python tools/corpus_bench.py --only kernels` gives
the per-kernel figures.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32 = 157.3e12
PEAK_HBM = 8.0e12


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


def bench_kernels(dev, out):
    from grafp_amd import ops
    n, secs, fs = 256, 30, 44100
    L = secs * fs
    x = torch.randn(n * L, device=dev) * 0.1
    lens = torch.full((n,), L, dtype=torch.int64)
    starts = torch.arange(n, dtype=torch.int64) * L
    res = ops.resample(x, starts, lens, fs, 16000)
    buf = res[0]
    _, _, _, taps = ops.resample_filter(fs, 16000)
    K = taps.shape[1]
    t = _events(lambda: ops.resample(x, starts, lens, fs, 16000, out=buf, out_starts=res[1]), 5)
    flops = 2.0 * K * buf.numel()
    out["resample"] = {"tracks": n, "seconds_each": secs, "K": K, "ms": t * 1e3, "tflops": flops / t / 1e12,
                       "fraction_of_f32_peak": flops / t / PEAK_F32}
    del x
    # draw_pairs: the resampled bank as the corpus (16 kHz, 30 s tracks)
    clip, om, B, A = 16000, 16800, 1024, 8
    norm = torch.ones(n, device=dev)
    rows = torch.randint(0, n, (B,), device=dev, dtype=torch.int32)
    u = torch.rand((B, A, 3), device=dev)
    t = _events(lambda: ops.draw_pairs(buf, res[1], res[2], norm, rows, u, clip, om, 0.0005), 20)
    nbytes = 4.0 * B * (om + 2 * clip)
    out["draw_pairs"] = {"pairs": B, "us": t * 1e6, "bytes": nbytes, "TBps": nbytes / t / 1e12,
                         "fraction_of_hbm_peak": nbytes / t / PEAK_HBM}


def _write_corpus(d, n, secs):
    rng = np.random.default_rng(0)
    for i in range(n):
        x = (0.1 * rng.standard_normal((secs * 44100, 2)) * 32767).astype("<i2")
        with wave.open(os.path.join(d, f"t{i:03d}.wav"), "wb") as w:
            w.setnchannels(2)
            w.setsampwidth(2)
            w.setframerate(44100)
            w.writeframes(x.tobytes())


def bench_load_and_step(dev, out, batch, steps):
    from grafp_amd.data import DeviceAudioCorpus
    from grafp_amd.train import Trainer, build_model, synthetic_batch
    from grafp_amd.util import load_config
    cfg = load_config()
    cfg["bsz_train"] = batch
    with tempfile.TemporaryDirectory() as d:
        _write_corpus(d, 48, 30)
        corpus = DeviceAudioCorpus(cfg, d, dev)
    out["load"] = dict(corpus.stats["load_s"], tracks=corpus.stats["tracks"], seconds=corpus.stats["seconds"])
    torch.manual_seed(0)
    model = build_model(cfg, device=dev)
    tr = Trainer(cfg, model, dev, amp_dtype=torch.bfloat16)
    x_i, x_j = synthetic_batch(batch, seed=100, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)

    def corpus_batch():
        rows = torch.randint(0, len(corpus.eligible), (batch,), generator=torch.Generator().manual_seed(1))
        return corpus._draw(rows.to(torch.int32), g, 8)

    for _ in range(3):
        tr.step_graph(x_i, x_j)
    torch.cuda.synchronize()
    res = {}
    for rep in range(2):                       # A/B/A/B: the two feeds alternate
        for name in ("synthetic", "corpus"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                a, b = corpus_batch() if name == "corpus" else (x_i, x_j)
                tr.step_graph(a, b)
            torch.cuda.synchronize()
            res.setdefault(name, []).append((time.perf_counter() - t0) / steps * 1e3)
    out["step_graph_ms"] = {k: min(v) for k, v in res.items()}
    out["step_graph_ms"]["corpus_over_synthetic"] = out["step_graph_ms"]["corpus"] / out["step_graph_ms"]["synthetic"]
    out["peak_memory_GiB"] = torch.cuda.max_memory_allocated(dev) / 2**30
    out["corpus_bank_GiB"] = corpus.bank.numel() * 4 / 2**30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["kernels", "all"], default="all")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    bench_kernels(dev, out)
    torch.cuda.empty_cache()
    if args.only == "all":
        bench_load_and_step(dev, out, args.batch, args.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
