"""What speed augmentation buys a briefly trained model (tests/test_gpu_speed.py runs this at 40
steps and gates only on what holds for any model).

Two models from the same initial weights, trained --steps steps each as tests/_retrieval_case.build_case trains (24 + 24
synthetic tracks, 64 pairs, lr 2e-4, bf16, white noise at 5 dB on the second view): one plain, one with speed_prob = 1 and
speed_range = [0.94, 1.06].  Then the protocol of section 12.22: 60 crops of 9 s per rho in 0.96, 1.0, 1.04 at 10 dB SNR,
speed changed through fs = round(16000 * rho), FingerprintLibrary.identify with and without tempo = 0.06.  Prints top-1
accuracy, the mean top-1 score and the winning ratios per model, and one JSON line.

  python tools/speed_aug_probe.py --steps 400
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

SPEED = {"speed_prob": 1.0, "speed_range": [0.94, 1.06]}


def train(cfg, pool, steps, dev, seed=0):
    """One model trained `steps` steps on crops of `pool`; with speed on the crops carry the resampler's context."""
    from _retrieval_case import add_noise
    from grafp_amd.train import Trainer, build_model
    torch.manual_seed(seed)
    model = build_model(cfg, device=dev)
    tr = Trainer(cfg, model, dev, amp_dtype=torch.bfloat16, lr=2e-4)
    L, pad = tr.draw_len, tr.augment.pad
    g = torch.Generator().manual_seed(seed + 1)
    losses = []
    for it in range(steps):
        ti = torch.randint(0, pool.shape[0], (64,), generator=g)
        off = torch.randint(0, pool.shape[1] - 16000, (64,), generator=g)
        # the clip starts at `off` as in build_case; its context is cut from the same track (shifted at the track's ends)
        lo = [min(max(b - pad, 0), pool.shape[1] - L) for b in off.tolist()]
        x_i = torch.stack([pool[a, b:b + L] for a, b in zip(ti.tolist(), lo)])
        losses.append(tr.step(x_i, add_noise(x_i, 5.0, 77 * it)))
    model.eval()
    return model, torch.stack(losses).float().cpu()


def protocol(model, cfg, tracks, say):
    from _retrieval_case import add_noise
    from grafp_amd.library import FingerprintLibrary
    lib = FingerprintLibrary.build(model, list(tracks), cfg)
    rng = np.random.RandomState(23)
    L = 9 * 16000 + 512
    rows = []
    for rho in (0.96, 1.0, 1.04):
        crops, truth = [], []
        for i in range(60):
            t = int(rng.randint(0, tracks.shape[0]))
            s0 = int(rng.randint(0, tracks.shape[1] - L))
            crops.append(tracks[t, s0:s0 + L])
            truth.append(t)
        noisy = list(add_noise(torch.stack(crops), 10.0, 41))
        fs = int(round(16000 * rho))
        plain = lib.identify(noisy, fs=fs)
        sloped = lib.identify(noisy, fs=fs, tempo=0.06)
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
    cfg = load_config()
    cfg["bsz_train"] = 64
    db_tracks = synth_tracks(24, 20, 1000, dev)
    pool = torch.cat([db_tracks, synth_tracks(24, 20, 5000, dev)])
    out = {"steps": steps}
    for name, extra in (("plain", {}), ("speed", SPEED)):
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
