"""What time-stretch augmentation buys a briefly trained model (tests/test_gpu_stretch.py runs this
at 40 steps and gates only on what holds for any model).

Two models from the same initial weights, trained --steps steps each as tools/speed_aug_probe.train does (24 + 24 synthetic
tracks, 64 pairs, lr 2e-4, bf16, white noise at 5 dB on the second view): one plain, one with stretch_prob = 1 and
stretch_range = [0.94, 1.06].  Then the protocol of section 12.23 with time-stretched queries: 60 crops per rho in 0.96,
1.0, 1.04, each stretched to 9 s with ops.time_stretch (tempo moved, pitch kept), white noise at 10 dB SNR,
FingerprintLibrary.identify with and without tempo = 0.06.  Prints top-1 accuracy, the mean top-1 score and the winning
ratios per model, and one JSON line.

  python tools/stretch_aug_probe.py --steps 400
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

STRETCH = {"stretch_prob": 1.0, "stretch_range": [0.94, 1.06]}


def protocol(model, cfg, tracks, say):
    from _retrieval_case import add_noise
    from grafp_amd import ops
    from grafp_amd.library import FingerprintLibrary
    lib = FingerprintLibrary.build(model, list(tracks), cfg)
    rng = np.random.RandomState(23)
    L = 9 * 16000 + 512
    rows = []
    for rho in (0.96, 1.0, 1.04):
        pad, T_in = ops.stretch_pad(rho), ops.stretch_input_len(L, rho)
        crops, truth = [], []
        for i in range(60):
            t = int(rng.randint(0, tracks.shape[0]))
            s0 = int(rng.randint(0, tracks.shape[1] - T_in))
            crops.append(tracks[t, s0:s0 + T_in])
            truth.append(t)
        played = ops.time_stretch(torch.stack(crops), rho, L, x_offset=pad)
        noisy = list(add_noise(played, 10.0, 41))
        plain = lib.identify(noisy, fs=16000)
        sloped = lib.identify(noisy, fs=16000, tempo=0.06)
        acc = [float(np.mean([bool(r) and r[0]["track"] == t for r, t in zip(res, truth)])) for res in (plain, sloped)]
        score = [float(np.mean([r[0]["score"] for r in res if r])) for res in (plain, sloped)]
        nums = np.array([r[0]["tempo_num"] for r in sloped if r])
        below = sum(1 for p, s in zip(plain, sloped) if p and not (s and s[0]["score"] >= p[0]["score"]))
        say(f"  rho={rho}: top-1 accuracy dense {acc[0]:.3f} tempo {acc[1]:.3f}; mean top-1 score dense {score[0]:.4f} "
            f"tempo {score[1]:.4f}; winning ratio mean {nums.mean():.1f} (true {256 * rho:.1f}), min {nums.min()} "
            f"max {nums.max()}")
        rows.append({"rho": rho, "acc_dense": acc[0], "acc_tempo": acc[1], "score_dense": score[0], "score_tempo": score[1],
                     "ratio_mean": float(nums.mean()), "ratio_min": int(nums.min()), "ratio_max": int(nums.max()),
                     "tempo_below_dense": below})
    return rows


def experiment(steps, dev, say=print):
    from _retrieval_case import synth_tracks
    from grafp_amd.util import load_config
    from tools.speed_aug_probe import train
    cfg = load_config()
    cfg["bsz_train"] = 64
    db_tracks = synth_tracks(24, 20, 1000, dev)
    pool = torch.cat([db_tracks, synth_tracks(24, 20, 5000, dev)])
    out = {"steps": steps}
    for name, extra in (("plain", {}), ("stretch", STRETCH)):
        c = dict(cfg, **extra)
        model, losses = train(c, pool, steps, dev)
        say(f"{name}: {steps} steps, loss {losses[0]:.4f} -> {losses[-1]:.4f}")
        out[name] = {"losses_finite": bool(torch.isfinite(losses).all()), "loss_first": float(losses[0]),
                     "loss_last": float(losses[-1]), "rows": protocol(model, c, db_tracks, say)}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    print(json.dumps(experiment(args.steps, torch.device("cuda:0"))))
