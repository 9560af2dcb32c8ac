"""Float64 references, error bars, case tables and planted defects of the augmentation tests (TEST INFRASTRUCTURE):
tests/test_augment_cpu.py pins them on the CPU against oracle/csrc/augment.c, tests/test_gpu_augment.py holds
grafp_amd/csrc/augment.hip (ir_convolve_kernel, mix_partial_kernel + mix_apply_kernel) to them on every clip.

The bars are DERIVED from the kernels' operation counts, u = 2^-24 being the unit roundoff of f32; none is a measurement.

Convolution.  want[t] = sum_{l <= min(t, L-1)} h[l] x[t-l] in float64 (np.convolve(x, h)[:T]) and S[t] the same sum over
absolute values.  The kernel forms every output as ONE chain of n_t = min(t, L-1) + 1 fused multiply-adds (taps beyond t meet
zeros and add nothing), one rounding each, so by the standard bound of a recursive inner product
    |got[t] - want[t]| <= gamma(n_t) S[t],    gamma(n) = n u / (1 - n u).
At n = 1 this is the rounding of one product (u / (1 + u) relative), so the bar is tight there.

Mix.  n[t] = rec[(off + t) mod nl], scale = (rms(x) / 10^e) / (rms(n) + 1e-8), want[t] = x[t] + scale n[t], all in float64; e is
the f32 quotient float32(snr) / float32(20) widened, the rounding the kernel makes too (correctly rounded division), so of
the exponent only powf's own error remains.  The kernel's scale:
  * each sum of squares: a thread's chain of at most MX_CHUNK / MX_THREADS = 16 fmas, 6 shuffle levels across the wave, 3 adds
    across the 4 waves, then nchunks sequential adds of the partial sums (mix_apply_kernel starts from 0): every term is
    non-negative, so the relative error of a sum is at most gamma(16 + 6 + 3 + nchunks) ~ (25 + nchunks) u;
  * the square root halves that: (25 + nchunks) u / 2 for each rms, (25 + nchunks) u for the two;
  * scalar operations, 8 u in all: the two divisions by T (u each, halved by the root: 1 u together), the two roots (2 u), powf
    (1 ulp = 2 u), the + 1e-8f (1 u, which also covers 1e-8f against 1e-8), the two quotients (2 u);
so |scale_got / scale - 1| <= eps_scale = (33 + nchunks) u to first order, and with the one rounding of the final fma
    |got[t] - want[t]| <= eps_scale |scale n[t]| + u |want[t]|.
(The errors of rms(n) are damped by rms(n) / (rms(n) + 1e-8) <= 1, which the bound does not use.)

Inputs are closed-form (tests/_hashfill.py).  The planted defects are applied to the REFERENCE's output, never to a kernel:
each must leave its bar at least tenfold somewhere, or the bar could not tell the kernel from that mistake."""
import functools
from collections import namedtuple

import numpy as np

from _hashfill import hash_normalish

# grafp_amd/csrc/augment.hip, `constexpr int NAME = ...;` (tests/test_augment_cpu.py parses the file and compares)
AC_THREADS, AC_R = 256, 8
AC_H = AC_THREADS * AC_R            # 2048: half a tile; a thread's packed accumulators hold outputs o and o + AC_H
AC_TT = 2 * AC_H                    # 4096 outputs per workgroup
AC_LC = 512                         # taps per LDS chunk
MX_THREADS = 256
MX_CHUNK = MX_THREADS * 16          # 4096 samples per workgroup of the mix
KERNEL_CONSTANTS = {"AC_THREADS": AC_THREADS, "AC_R": AC_R, "AC_H": AC_H, "AC_TT": AC_TT, "AC_LC": AC_LC,
                    "MX_THREADS": MX_THREADS, "MX_CHUNK": MX_CHUNK}

U = 2.0 ** -24
PAD = 1000.0                        # what the padded (n, Lmax) banks hold behind a recording: never to be read


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def worst_ratio(err, bar):
    """max err / bar; an error where the bar is 0 (or a NaN) counts as infinite."""
    err, bar = np.asarray(err, np.float64).reshape(-1), np.asarray(bar, np.float64).reshape(-1)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)
    return float(np.nan_to_num(r, nan=np.inf).max())


# ---- convolution ---------------------------------------------------------------------------------------------------------
# Every case is ONE launch: clip i convolves with recording i of a ragged bank (lengths Ls), one more clip has index -1.
# tiles / last / upper: workgroups per clip, outputs of the last tile, and how many of those the .y halves store.
# reach[L]: per tile (ascending t0), (which side of `l_end = L < t0 + AC_TT ? L : t0 + AC_TT` holds, LDS chunks walked, taps of
# the recording in the last chunk -- below AC_LC means the chunk is zero-padded).  Hand-derived; the CPU test recomputes them.
ConvCase = namedtuple("ConvCase", "name T Ls tiles last upper reach")
_L1 = (("L", 1, 1),)
CONV_CASES = [
    # one output; L > T below one tile
    ConvCase("one-thread-1", 1, (1, 9), 1, 1, 0, {1: _L1, 9: (("L", 1, 9),)}),
    ConvCase("one-thread-8", 8, (1, 9), 1, 8, 0, {1: _L1, 9: (("L", 1, 9),)}),
    # one output past the half-tile: the .y store bound; the 8-tap step at 8 | 9; one chunk + 1 tap
    ConvCase("half-seam", 2049, (1, 8, 9, 513), 1, 2049, 1,
             {1: _L1, 8: (("L", 1, 8),), 9: (("L", 1, 9),), 513: (("L", 2, 1),)}),
    # full tiles and whole chunks only
    ConvCase("tile-exact-1", 4096, (512, 1024), 1, 4096, 2048, {512: (("L", 1, 512),), 1024: (("L", 2, 512),)}),
    ConvCase("tile-exact-2", 8192, (512, 1024), 2, 4096, 2048, {512: (("L", 1, 512),) * 2, 1024: (("L", 2, 512),) * 2}),
    # a last tile of one output; L = t0 + AC_TT on tile 0 (the clamp's `tile` side at equality) and 1 above; L > T
    ConvCase("tile-seam", 4097, (512, 4096, 4097, 6000), 2, 1, 0,
             {512: (("L", 1, 512),) * 2, 4096: (("tile", 8, 512), ("L", 8, 512)), 4097: (("tile", 8, 512), ("L", 9, 1)),
              6000: (("tile", 8, 512), ("L", 12, 368))}),
    # zero-padded last chunks (511, 513, 10243), L = t0 + AC_TT on tile 1, L = T
    ConvCase("three-tiles", 10243, (511, 513, 8192, 10243), 3, 2051, 3,
             {511: (("L", 1, 511),) * 3, 513: (("L", 2, 1),) * 3,
              8192: (("tile", 8, 512), ("tile", 16, 512), ("L", 16, 512)),
              10243: (("tile", 8, 512), ("tile", 16, 512), ("L", 21, 3))}),
]
CONV_BY_NAME = {c.name: c for c in CONV_CASES}


def conv_reach(T, L):
    """What ir_convolve_kernel does with a recording of L taps on a clip of T samples, from the constants: (tiles, outputs of
    the last tile, outputs its .y halves store, per tile (clamp side, chunks, taps in the last chunk))."""
    tiles = -(-T // AC_TT)
    last = T - (tiles - 1) * AC_TT
    per_tile = []
    for k in range(tiles):
        t0 = k * AC_TT
        side, l_end = ("L", L) if L < t0 + AC_TT else ("tile", t0 + AC_TT)
        chunks = -(-l_end // AC_LC)
        per_tile.append((side, chunks, min(L, chunks * AC_LC) - (chunks - 1) * AC_LC))
    return tiles, last, max(0, last - AC_H), tuple(per_tile)


def conv_inputs(case):
    """x (B, T) f32, the recordings (list of f32 arrays), ir_index (B) int32: clip i takes recording i, the last clip none."""
    n = len(case.Ls)
    x = (0.5 * hash_normalish(f"aug:{case.name}.x", (n + 1, case.T))).astype(np.float32)
    recs = [(hash_normalish(f"aug:{case.name}.h{i}", (L,)) / np.sqrt(L)).astype(np.float32) for i, L in enumerate(case.Ls)]
    return x, recs, np.array(list(range(n)) + [-1], np.int32)


def ragged(recs):
    """(flat f32 buffer, starts int64, lens int32): the recordings back to back, what load_bank produces."""
    lens = np.array([r.size for r in recs], np.int32)
    starts = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
    return np.concatenate(recs).astype(np.float32), starts, lens


def padded(recs):
    """(n, Lmax) f32 rows; behind a recording the row holds PAD, which nothing may read."""
    bank = np.full((len(recs), max(r.size for r in recs)), PAD, np.float32)
    for i, r in enumerate(recs):
        bank[i, :r.size] = r
    return bank


def conv_ref(x_row, h):
    """(want, bar) of one clip in float64."""
    T, L = x_row.size, h.size
    x64, h64 = x_row.astype(np.float64), h.astype(np.float64)
    want = np.convolve(x64, h64)[:T]
    S = np.convolve(np.abs(x64), np.abs(h64))[:T]
    return want, gamma(np.minimum(np.arange(T), L - 1) + 1) * S


@functools.lru_cache(maxsize=None)
def cached_conv(name):
    """(x, recs, idx), (want (B, T) float64, bar (B, T) float64) of a case, computed once per process, read-only.  The skipped
    clip's want is its input and its bar 0 (the tests compare its BITS)."""
    case = CONV_BY_NAME[name]
    x, recs, idx = conv_inputs(case)
    want, bar = np.empty(x.shape, np.float64), np.zeros(x.shape, np.float64)
    for b, i in enumerate(idx):
        want[b], bar[b] = conv_ref(x[b], recs[i]) if i >= 0 else (x[b].astype(np.float64), 0.0)
    for a in [x, idx, want, bar] + recs:
        a.setflags(write=False)
    return (x, tuple(recs), idx), (want, bar)


def conv_excess(got, name):
    """Worst |got - want| / bar over the convolved clips of a case (got: (B, T) f32)."""
    (_, _, idx), (want, bar) = cached_conv(name)
    on = idx >= 0
    return worst_ratio(np.abs(got[on].astype(np.float64) - want[on]), bar[on])


def _conv_defect_row(defect, x_row, h, want_row):
    T, L = x_row.size, h.size
    x64, h64 = x_row.astype(np.float64), h.astype(np.float64)
    out = want_row.copy()
    if defect == "last-tap-dropped":
        out[L - 1:] -= h64[L - 1] * x64[:max(0, T - L + 1)]
    elif defect == "x0-before-the-start":              # taps l > t meet x[0] instead of 0
        tail = np.concatenate([np.cumsum(h64[::-1])[::-1], [0.0]])          # tail[k] = sum_{l >= k} h[l]
        out += x64[0] * tail[np.minimum(np.arange(T) + 1, L)]
    elif defect == "taps-from-512-shifted":            # tap l >= AC_LC meets x[t - l - 1]
        if L > AC_LC:
            late = np.concatenate([np.zeros(AC_LC), h64[AC_LC:]])
            out += np.convolve(x64, np.concatenate([[0.0], late]))[:T] - np.convolve(x64, late)[:T]
    elif defect == "upper-half-shifted":               # output t of an upper half-tile holds output t - 1
        t = np.arange(T)
        up = (t % AC_TT) >= AC_H
        out[up] = want_row[t[up] - 1]
    elif defect == "stale-last-output":                # a partial tile never stores output T - 1
        if T % AC_TT:
            out[T - 1] = 0.0
    else:
        raise KeyError(defect)
    return out


CONV_DEFECTS = ["last-tap-dropped", "x0-before-the-start", "taps-from-512-shifted", "upper-half-shifted", "stale-last-output",
                "neighbours-recording"]


def conv_defect_excess(defect, name):
    """Worst (defective reference - reference) / bar of a case."""
    (x, recs, idx), (want, bar) = cached_conv(name)
    worst = 0.0
    for b, i in enumerate(idx):
        if i < 0:
            continue
        if defect == "neighbours-recording":
            bad = conv_ref(x[b], recs[(i + 1) % len(recs)])[0]
        else:
            bad = _conv_defect_row(defect, x[b], recs[i], want[b])
        worst = max(worst, worst_ratio(np.abs(bad - want[b]), bar[b]))
    return worst


# ---- mix -----------------------------------------------------------------------------------------------------------------
# Every case is ONE launch of 5 clips: clips 0-3 read recording 1 of a two-recording bank (recording 0 is a decoy of 37
# samples) from `off` at the four SNRs, clip 4 has index -1.  kind: "quiet" scales the recording to an rms of 1e-7 (the
# + 1e-8 is then ~10 % of the denominator), "zero-signal" / "zero-noise" zero x / the recording (out == x).
# chunks / last / step: workgroups per clip, samples of the last one, and the circular pointer's stride MX_THREADS % nl.
MixCase = namedtuple("MixCase", "name T nl off kind chunks last step")
MIX_SNRS = (-5.0, 0.0, 7.3, 30.0)
MIX_CASES = [
    MixCase("one-sample", 1, 1, 0, "plain", 1, 1, 0),
    MixCase("nl-2", 255, 2, 1, "plain", 1, 255, 0),
    MixCase("nl-255", 257, 255, 254, "plain", 1, 257, 1),
    MixCase("nl-chunk", 4096, 4096, 4095, "plain", 1, 4096, 256),
    MixCase("nl-256", 4097, 256, 255, "plain", 2, 1, 0),
    MixCase("nl-257-offset-beyond", 4097, 257, 300, "plain", 2, 1, 256),        # off >= nl: the kernel reduces it
    MixCase("nl-above-T", 8195, 9000, 8999, "plain", 3, 3, 256),
    MixCase("nl-T", 8195, 8195, 1, "plain", 3, 3, 256),
    MixCase("four-chunks", 12289, 4096, 7, "plain", 4, 1, 256),
    MixCase("quiet-recording", 8195, 9000, 8999, "quiet", 3, 3, 256),
    MixCase("zero-signal", 4097, 257, 300, "zero-signal", 2, 1, 256),
    MixCase("zero-noise", 4097, 257, 300, "zero-noise", 2, 1, 256),
]
MIX_BY_NAME = {c.name: c for c in MIX_CASES}
QUIET_RMS = 1e-7


def mix_reach(T, nl):
    chunks = -(-T // MX_CHUNK)
    return chunks, T - (chunks - 1) * MX_CHUNK, MX_THREADS % nl


def mix_inputs(case):
    """x (5, T) f32, the two recordings, noise_index, noise_offset (int32), snr_db (f32)."""
    x = (0.1 * hash_normalish(f"aug:{case.name}.x", (5, case.T))).astype(np.float32)
    rec = (0.3 * hash_normalish(f"aug:{case.name}.n", (case.nl,))).astype(np.float32)
    if case.kind == "quiet":
        rec = (rec.astype(np.float64) * (QUIET_RMS / np.sqrt((rec.astype(np.float64) ** 2).mean()))).astype(np.float32)
    elif case.kind == "zero-signal":
        x = np.zeros_like(x)
    elif case.kind == "zero-noise":
        rec = np.zeros_like(rec)
    decoy = hash_normalish(f"aug:{case.name}.decoy", (37,)).astype(np.float32)
    idx = np.array([1, 1, 1, 1, -1], np.int32)
    off = np.array([case.off] * 4 + [0], np.int32)
    snr = np.array(MIX_SNRS + (10.0,), np.float32)
    return x, [decoy, rec], idx, off, snr


MIX_DEFECTS = ["offset-plus-1", "rms-over-the-recording", "no-1e-8", "last-chunk-dropped", "snr-sign-flipped"]


def mix_ref(x_row, rec, off, snr, defect=None):
    """(want, bar) of one clip in float64; with `defect` the want of that mistake (a planted defect: see the module)."""
    T, nl = x_row.size, rec.size
    x64, r64 = x_row.astype(np.float64), rec.astype(np.float64)
    n = r64[(int(off) + (1 if defect == "offset-plus-1" else 0) + np.arange(T, dtype=np.int64)) % nl]
    chunks = -(-T // MX_CHUNK)
    upto = (chunks - 1) * MX_CHUNK if defect == "last-chunk-dropped" else T
    sx, sn = (x64[:upto] ** 2).sum(), (n[:upto] ** 2).sum()
    rms_x = np.sqrt(sx / T)
    rms_n = np.sqrt((r64 ** 2).mean()) if defect == "rms-over-the-recording" else np.sqrt(sn / T)
    e = float(np.float32(snr) / np.float32(20.0))
    if defect == "snr-sign-flipped":
        e = -e
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = (rms_x / 10.0 ** e) / (rms_n + (0.0 if defect == "no-1e-8" else 1e-8))
        want = x64 + scale * n
        return want, (33 + chunks) * U * np.abs(scale * n) + U * np.abs(want)


@functools.lru_cache(maxsize=None)
def cached_mix(name):
    """(x, recs, idx, off, snr), (want (5, T), bar (5, T)) of a case; the skipped clip's want is its input, its bar 0."""
    x, recs, idx, off, snr = mix_inputs(MIX_BY_NAME[name])
    want, bar = np.empty(x.shape, np.float64), np.zeros(x.shape, np.float64)
    for b, i in enumerate(idx):
        want[b], bar[b] = mix_ref(x[b], recs[i], off[b], snr[b]) if i >= 0 else (x[b].astype(np.float64), 0.0)
    for a in [x, idx, off, snr, want, bar] + recs:
        a.setflags(write=False)
    return (x, tuple(recs), idx, off, snr), (want, bar)


def mix_excess(got, name):
    """Worst |got - want| / bar over the mixed clips of a case (got: (5, T) f32)."""
    (_, _, idx, _, _), (want, bar) = cached_mix(name)
    on = idx >= 0
    return worst_ratio(np.abs(got[on].astype(np.float64) - want[on]), bar[on])


def mix_defect_excess(defect, name):
    (x, recs, idx, off, snr), (want, bar) = cached_mix(name)
    worst = 0.0
    for b, i in enumerate(idx):
        if i >= 0:
            bad = mix_ref(x[b], recs[i], off[b], snr[b], defect)[0]
            worst = max(worst, worst_ratio(np.abs(bad - want[b]), bar[b]))
    return worst


def assert_defect_shows(excess_of, defect, names, must_show_on=()):
    """The planted defect leaves the bar at least tenfold on at least one case, and on every case of must_show_on."""
    seen = {name: excess_of(defect, name) for name in names}
    assert max(seen.values()) >= 10.0, (defect, seen)
    for name in must_show_on:
        assert seen[name] >= 10.0, (defect, name, seen[name])
    return seen
