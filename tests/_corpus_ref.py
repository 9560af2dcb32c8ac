"""CPU restatements of the device corpus kernels (csrc/corpus.hip) for tests/test_gpu_corpus.py and tools/corpus_bench.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def taps_f64(orig_fs, new_fs):
    """(orig, new, width, taps (new, K) float64) of torchaudio's default Resample filter, evaluated in f64."""
    g = math.gcd(orig_fs, new_fs)
    orig, new = orig_fs // g, new_fs // g
    base = min(orig, new) * 0.99
    width = math.ceil(6 * orig / base)
    k = (np.arange(2 * width + orig) - width)[None, :] / orig
    t = np.clip((-np.arange(new)[:, None] / new + k) * base, -6.0, 6.0)
    w = np.cos(t * math.pi / 12) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0, 1.0, np.sin(math.pi * t) / (math.pi * t))
    return orig, new, width, s * w * base / orig


def resample_f64(x, orig_fs, new_fs):
    """out[j*new + p] = sum_k tap[p][k] * x[j*orig + k - width] in f64, zeros outside the track."""
    orig, new, width, taps = taps_f64(orig_fs, new_fs)
    x = np.asarray(x, dtype=np.float64)
    L, K = x.size, taps.shape[1]
    M = -(-new * L // orig)
    nJ = -(-M // new)
    xp = np.concatenate([np.zeros(width), x, np.zeros(nJ * orig + K)])
    X = xp[np.arange(nJ)[:, None] * orig + np.arange(K)[None, :]]
    return (X @ taps.T).reshape(-1)[:M]


def resample_torch_f32(x, orig_fs, new_fs):
    """torchaudio's own computation restated on torch CPU: F.pad + conv1d(stride=orig) with the f32 taps."""
    from grafp_amd.ops import resample_filter
    orig, new, width, taps = resample_filter(orig_fs, new_fs)
    x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    L = x.numel()
    y = F.conv1d(F.pad(x.view(1, 1, -1), (width, width + orig)), torch.from_numpy(taps)[:, None, :], stride=orig)
    return y[0].t().reshape(-1)[:-(-new * L // orig)]


def draw_pairs_ref(tracks, norms, row_track, uniforms, clip, offset_mod, silence):
    """The kernel's contract on torch CPU: tracks = list of 1-D f32 tensors (the eligible tracks, in order)."""
    B, A, _ = uniforms.shape
    n = len(tracks)
    x_i, x_j = torch.empty(B, clip), torch.empty(B, clip)
    silent_rows = 0

    def pick(u, m):
        return min(int(math.floor(float(u) * m)), m - 1)
    for b in range(B):
        for a in range(A):
            t = (int(row_track[b]) + a) % n
            y = tracks[t]
            u = uniforms[b, a].double()
            r = pick(u[0], y.numel() - offset_mod)
            ri, rj = pick(u[1], offset_mod - clip), pick(u[2], offset_mod - clip)
            ci, cj = y[r + ri:r + ri + clip], y[r + rj:r + rj + clip]
            silent = bool(ci.abs().max() < silence) or bool(cj.abs().max() < silence)
            if not silent or a == A - 1:
                x_i[b], x_j[b] = ci / norms[t], cj / norms[t]
                silent_rows += int(silent)
                break
    return x_i, x_j, silent_rows
