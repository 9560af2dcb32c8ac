"""CPU restatements of the device corpus kernels (csrc/corpus.hip) and the table of resample launch plans, for
tests/test_corpus_cpu.py, tests/test_gpu_corpus.py and tools/corpus_bench.py."""
import collections
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


# ---- the resample launch plan, as grafp_resample_plan reports it --------------------------------------------------------
# resample_launch (csrc/corpus.hip): n_pb = ceil(new / 10) phase blocks; JT = ceil(16 / n_pb) tiles of 64 output blocks per
# workgroup, lowered one at a time until the window W = (64*JT - 1)*orig + K4 fits the LDS_FLOATS of a CU; refused when even
# JT = 1 does not fit.  ops.resample only uses the ratio, so small integers are legal rates.  JT and n_pb below are worked out
# by hand from that rule (K = 2*width + orig, width = ceil(6*orig / (0.99*min(orig, new))), K4 = K rounded up to 4):
#   441/160 K 475;  3/1 K 41;  441/320 K 459;  2/1 K 28;  1/2 K 15;  441/640 K 455       the six rates of the first tests
#   441/80   K 509 K4 512: JT 2 needs 127*441 + 512 = 56 519 > 40 960 -> 1
#   441/40   K 575 K4 576: JT 4, 3, 2 do not fit -> 1
#   49/8     K 125 K4 128: JT 16 needs 50 255, 14 needs 43 983, 13 needs 831*49 + 128 = 40 847 <= 40 960 (452 bytes to spare)
#   147/25   K 219 K4 220: JT 6 needs 56 521, 5 needs 47 113, 4 needs 255*147 + 220 = 37 705
#   15/16    K 29;  7/33 K 21;  160/441 K 174: no shrink
#   640/1    K 8398 K4 8400: JT 1 needs 63*640 + 8400 = 48 720;  1000/1 K 13 122 K4 13 124: 76 124           -> refused
LDS_FLOATS = 160 * 1024 // 4
PHASES = 10
Case = collections.namedtuple("Case", "orig_fs new_fs JT n_pb reaches")
RESAMPLE_CASES = (
    Case(44100, 16000, 1, 16, ""),
    Case(48000, 16000, 16, 1, ""),
    Case(22050, 16000, 1, 32, ""),
    Case(32000, 16000, 16, 1, ""),
    Case(8000, 16000, 16, 1, ""),
    Case(11025, 16000, 1, 64, ""),
    Case(44100, 8000, 1, 8, "shrink"),
    Case(176400, 16000, 1, 4, "shrink"),
    Case(49, 8, 13, 1, "shrink intermediate near_full ragged"),
    Case(147, 25, 4, 3, "shrink intermediate ragged"),
    Case(15, 16, 8, 2, "intermediate ragged"),
    Case(7, 33, 4, 4, "intermediate ragged"),
    Case(16000, 44100, 1, 45, "ragged"),
)
RESAMPLE_REFUSED = ((640, 1, 48720), (1000, 1, 76124))          # (orig_fs, new_fs, the window the message names)
Plan = collections.namedtuple("Plan", "JT n_pb K4 W lds_bytes blocks tile_in")


def case_id(c):
    return f"{c.orig_fs}to{c.new_fs}"


def resample_plan(lib, orig_fs, new_fs):
    """(status, Plan, message) of grafp_resample_plan for the filter ops.resample builds for the rate pair."""
    import ctypes
    from grafp_amd.ops import resample_filter
    orig, new, width, taps = resample_filter(orig_fs, new_fs)
    info = (ctypes.c_int * 8)()
    rc = lib.grafp_resample_plan(orig, new, width, taps.shape[1], info)
    assert info[7] == 0
    return rc, Plan(*info[:7]), lib.grafp_last_error().decode() if rc else ""


def case_lengths(plan, orig, K):
    """Input lengths around the workgroup tile of T = 64*JT*orig input samples: none, one sample, less than a filter, one
    sample short of n_j = 64*JT output blocks, exactly that, one block more, and two tiles plus a block plus one sample."""
    T = 64 * plan.JT * orig
    assert T == plan.tile_in
    return [0, 1, K - 1, T - 1, T, T + 1, 2 * T + orig + 1]


# ---- the training draw ------------------------------------------------------------------------------------------------
def draw_pairs_ref(tracks, norms, row_track, uniforms, clip, offset_mod, silence, branches=False):
    """The kernel's whole contract on torch CPU: tracks = list of 1-D f32 tensors (the tracks of the launch, in order).
    A track with len - offset_mod < 1 takes r = 0 and reads zeros past its end; attempt a of row b uses track
    (row_track[b] + a) mod n (Python's sign rule, so -1 is the last track); `silence` is the f32 the kernel receives and
    the comparison is a strict <.  branches=True: also returns a Counter of the branches taken."""
    B, A, _ = uniforms.shape
    n = len(tracks)
    x_i, x_j = torch.empty(B, clip), torch.empty(B, clip)
    silent_rows = 0
    taken = collections.Counter()
    silence = float(np.float32(silence))

    def pick(u, m, slot):
        f = int(math.floor(float(u) * m))
        taken[f"u{slot}_zero"] += float(u) == 0.0
        taken[f"u{slot}_last_below_one"] += float(u) == float(np.nextafter(np.float32(1), np.float32(0)))
        taken[f"u{slot}_clamped"] += f > m - 1
        return min(f, m - 1)

    def crop(y, s):
        c = y[s:s + clip]                                  # slicing past the end gives fewer (or no) samples
        taken["zero_padded"] += c.numel() < clip
        return F.pad(c, (0, clip - c.numel()))
    for b in range(B):
        t0 = int(row_track[b])
        taken["row_negative"] += t0 < 0
        taken["row_past_n"] += t0 >= n
        for a in range(A):
            t = (t0 + a) % n
            y = tracks[t]
            u = uniforms[b, a].double()
            m = y.numel() - offset_mod
            taken["short_track"] += m < 1
            r = pick(u[0], m, 0) if m >= 1 else 0
            ri, rj = pick(u[1], offset_mod - clip, 1), pick(u[2], offset_mod - clip, 2)
            ci, cj = crop(y, r + ri), crop(y, r + rj)
            pi, pj = float(ci.abs().max()), float(cj.abs().max())
            silent = pi < silence or pj < silence
            taken["peak_equals_silence"] += not silent and (pi == silence or pj == silence)
            if not silent or a == A - 1:
                x_i[b], x_j[b] = ci / norms[t], cj / norms[t]
                silent_rows += int(silent)
                taken["exhausted" if silent else "accepted_first" if a == 0 else "accepted_later"] += 1
                break
            taken["rejected"] += 1
    taken = +taken                                             # drop the branches never taken
    return (x_i, x_j, silent_rows, taken) if branches else (x_i, x_j, silent_rows)


def quantile_f64(v, q):
    """Linear-interpolation quantile on the sorted float64 copies of the values: rank r = q (n - 1) in f64."""
    s = np.sort(np.asarray(v, dtype=np.float64))
    r = q * (s.size - 1)
    lo = int(math.floor(r))
    hi = min(lo + 1, s.size - 1)
    return s[lo] + (s[hi] - s[lo]) * (r - lo)


def quantile_bracket(s, q):
    """[low, high] for data._quantile past 2^24 elements, s = the sorted values: the order statistics at floor(r) - 3 and
    floor(r) + 4 of the f64 rank r = q (n - 1).  Derived: past 2^24 the f32 rank is an integer at most 1 from the f32
    product, the f32 rounding of q moves it by at most 1 more ((n - 1) * 2^-25 < 1 for n < 2^25), and ceil adds 1."""
    lo = int(math.floor(q * (len(s) - 1)))
    return float(s[max(lo - 3, 0)]), float(s[min(lo + 4, len(s) - 1)])

