"""CPU restatements of grafp_time_stretch_f32 (csrc/stretch.hip) for tests/test_stretch_cpu.py, tests/test_gpu_stretch.py
and tools/stretch_bench.py: the rule (WSOLA) in float64 with every candidate's correlation and the f32 error bound of
each frame, and the kernel's output arithmetic in numpy float32, operation by operation.

An arg-max cannot be held to a tolerance, so the tests follow the kernel: `check_shifts` walks the path of the kernel's own
shifts and asks of each frame that its choice be within the frame's bound of the best candidate, and equal to the rule's
winner wherever that winner leads by more than the bound (a "certified" frame)."""
import functools
from collections import namedtuple

import numpy as np

F32 = np.float32
N, HS, D = 512, 256, 128                 # ST_N, ST_HS, ST_D
PI_N = F32(0.00613592315154256491887)    # ST_PI_N
EPS = 2.0 ** -24

Stretch = namedtuple("Stretch", "out shifts corr bound lead first")
# out    (T_out,) outputs (only those of the frames walked are filled; the others are 0)
# shifts (F,) the path walked: the rule's own winners, or the shifts given
# corr   (F, 256) float64 correlations c(delta), column delta + 128; rows of frames not walked (and row 0) are 0
# bound  (F,) 2 N 2^-24 max over delta of sum |t[n]| |xz[a_i + delta + n]|
# lead   (F,) the rule's winner's lead over the runner-up (inf where every product is zero: nothing to round)
# first  the first frame walked


def clamp_ratio(r):
    """The kernels' warp_ratio (csrc/clipwarp.h) on an f32: NaN -> 1, then [0.5, 2]."""
    r = F32(r)
    if r != r:
        return F32(1.0)
    return F32(0.5) if r < F32(0.5) else (F32(2.0) if r > F32(2.0) else r)


def frames(T_out):
    return -(-int(T_out) // HS) + 1


def position(i, rho, x_offset):
    """a_i: rho is the f32 ratio's value as a Python float; (i - 1) * HS * rho is exact in f64."""
    return int(x_offset) + int(np.floor((i - 1) * HS * float(rho) + 0.5))


def _xz(x, s, n):
    """xz[s .. s + n): x inside [0, len), 0 outside."""
    out = np.zeros(n, dtype=x.dtype)
    lo, hi = max(s, 0), min(s + n, x.size)
    if hi > lo:
        out[lo - s:hi - s] = x[lo:hi]
    return out


def winner(c):
    """The rule's choice among the 256 correlations: the largest; ties to the smaller |delta|, then the negative one."""
    d = np.flatnonzero(c == c.max()) - D
    return int(d[np.lexsort((d, np.abs(d)))][0])


def stretch_f64(x, rho, T_out, x_offset=0, shifts=None, first=1, copy_at_one=True):
    """The rule in float64 for one clip -> Stretch.  rho: a float, used as given after the clamp (the GPU tests pass the
    f32 ratio's value).  shifts: walk this path instead of the rule's own winners (the correlations and bounds are then
    those the kernel saw).  first > 1 (needs shifts): only frames first .. F - 1 and their outputs are computed.
    copy_at_one=False runs the frames at rho == 1 too instead of the rule's copy."""
    rho = float(rho)
    rho = 1.0 if rho != rho else min(max(rho, 0.5), 2.0)
    x = np.asarray(x, dtype=np.float64)
    F = frames(T_out)
    out, corr, bound = np.zeros((F - 1) * HS), np.zeros((F, 2 * D)), np.zeros(F)
    lead, path = np.full(F, np.inf), np.zeros(F, dtype=np.int64)
    if rho == 1.0 and copy_at_one:
        return Stretch(_xz(x, int(x_offset), int(T_out)), path, corr, bound, lead, 1)
    assert first == 1 or shifts is not None
    w = np.sin(np.pi * np.arange(N) / N) ** 2
    if shifts is not None:
        path[:] = np.asarray(shifts, dtype=np.int64)
        assert path[0] == 0
    for i in range(first, F):
        a = position(i, rho, x_offset)
        t = _xz(x, position(i - 1, rho, x_offset) + int(path[i - 1]) + HS, N)
        reg = _xz(x, a - D, N + 2 * D - 1)
        win = np.lib.stride_tricks.sliding_window_view(reg, N)                 # (256, 512): row delta + 128
        corr[i] = win @ t
        bound[i] = 2 * N * EPS * (np.abs(win) @ np.abs(t)).max()
        if bound[i] > 0:
            top = np.sort(corr[i])
            lead[i] = top[-1] - top[-2]
        if shifts is None:
            path[i] = winner(corr[i])
        cur = _xz(x, a + int(path[i]), HS)
        out[(i - 1) * HS:i * HS] = w[HS:] * t[:HS] + w[:HS] * cur
    return Stretch(out[:T_out], path, corr, bound, lead, first)


def certified(ref):
    """Per frame walked: does the rule's winner lead the runner-up by more than the f32 bound?  (Where every product of
    a frame is zero -- its template or its whole search region lies in the padding -- every c is exactly 0 in any
    arithmetic and the tie rule alone decides: such a frame counts as certified.)"""
    ok = ref.lead > ref.bound
    ok[:ref.first] = True
    return ok


def check_shifts(x, rho, T_out, x_offset, shifts, first=1):
    """What the tests ask of a kernel's shifts, along the kernel's own path: c64(delta_i) >= max c64 - bound_i, and
    delta_i equal to the rule's winner wherever the frame is certified.  -> the float64 Stretch on that path."""
    shifts = np.asarray(shifts, dtype=np.int64)
    ref = stretch_f64(x, rho, T_out, x_offset, shifts=shifts, first=first)
    if float(clamp_ratio(rho)) == 1.0:
        assert not shifts.any()
        return ref
    assert shifts[0] == 0 and shifts.min() >= -D and shifts.max() < D
    ok = certified(ref)
    for i in range(first, shifts.size):
        c = ref.corr[i]
        assert c[shifts[i] + D] >= c.max() - ref.bound[i], (i, int(shifts[i]), winner(c), c[shifts[i] + D], c.max(), ref.bound[i])
        if ok[i]:
            assert shifts[i] == winner(c), (i, int(shifts[i]), winner(c))
    return ref


def stretch_f32(x, rho, T_out, x_offset, shifts, first=1):
    """The kernel's output arithmetic in numpy f32 on a given path: sn = sinf(n * pi/N), cs = cosf(n * pi/N) with the
    angle formed in f32; out = (cs * cs) * xz[p_{i-1} + HS + n] + (sn * sn) * xz[p_i + n], two products and one sum,
    each rounded to f32.  rho == 1: the copy."""
    r = clamp_ratio(rho)
    x = np.asarray(x, dtype=F32)
    if r == F32(1.0):
        return _xz(x, int(x_offset), int(T_out))
    F = frames(T_out)
    out = np.zeros((F - 1) * HS, dtype=F32)
    ang = np.arange(HS, dtype=F32) * PI_N
    sn, cs = np.sin(ang), np.cos(ang)
    w_new, w_old = sn * sn, cs * cs
    assert w_new.dtype == F32 and ang.dtype == F32
    for i in range(first, F):
        old = _xz(x, position(i - 1, float(r), x_offset) + int(shifts[i - 1]) + HS, HS)
        cur = _xz(x, position(i, float(r), x_offset) + int(shifts[i]), HS)
        out[(i - 1) * HS:i * HS] = w_old * old + w_new * cur
    return out[:T_out]


# ---- case generators ---------------------------------------------------------------------------------------------
SMALL_RATIOS = np.array([0.5, 0.94, 1.0, np.nextafter(F32(1.0), F32(2.0)), 1.06, 2.0], dtype=F32)


def music(T, seed):
    """(T,) f32: six sinusoids in 80-3 000 Hz at fs = 16 000 plus 5 % white noise, normalised to peak 1.  Tonal input
    gives the correlation a clear peak; which seeds certify every frame is checked in tests/test_stretch_cpu.py."""
    r = np.random.default_rng(seed)
    t = np.arange(T) / 16000.0
    x = np.zeros(T)
    for f in r.uniform(80, 3000, 6):
        x += r.uniform(0.2, 1) * np.sin(2 * np.pi * f * t + r.uniform(0, 6.28))
    x += 0.05 * r.standard_normal(T)
    return (x / np.abs(x).max()).astype(F32)


def music_rows(T, seeds):
    """(len(seeds), T): one row per seed."""
    return np.stack([music(T, s) for s in seeds])


T_SMALL = 1300                           # not a multiple of the hop: 7 frames, the last one covers 20 outputs
SMALL_SEEDS = (0, 4, 6, 7, 2, 3)         # one per row; tests/test_stretch_cpu.py checks that every frame is certified
LONG_RATIOS = np.array([1.06, 0.94, 0.97], dtype=F32)
LONG_SEEDS = (0, 4, 6)
LONG_TAIL = (16, 16, 160)                # frames checked at the end of each row: at 0.97 an f32 position is off by one
#                                          sample at frames 1065, 1090, ... 1190 of the 1210 (tests/test_stretch_cpu.py)
LONG_T_IN = 300000


@functools.lru_cache(maxsize=None)
def small_cases():
    """Case 1 of tests/test_gpu_stretch.py, six clips at SMALL_RATIOS, with the rule's float64 result per row:
    "inside": T_in = stretch_input_len(1300, 2), x_offset = pad, no read in the padding at any ratio;
    "edges": the first 900 samples from x_offset = 0: frame 0 and the last frames read padding, the tail is zeros.
    -> {name: (x, x_offset, [Stretch per row])}; computed once and shared, not to be written to."""
    from grafp_amd import ops
    pad, T_in = ops.stretch_pad(2.0), ops.stretch_input_len(T_SMALL, 2.0)
    x = music_rows(T_in, SMALL_SEEDS)
    cases = {}
    for name, xs, off in (("inside", x, pad), ("edges", np.ascontiguousarray(x[:, :900]), 0)):
        xs.setflags(write=False)
        cases[name] = (xs, off, [stretch_f64(row, float(r), T_SMALL, off) for row, r in zip(xs, SMALL_RATIOS)])
    return cases


@functools.lru_cache(maxsize=None)
def long_case():
    """Case 5: rows of 300 000 input samples from x_offset = 0 at 1.06, 0.94 and 0.97, as many outputs as the input gives
    (over 1 100 frames) -> (x, [T_out per row], [Stretch per row] on the rule's own path)."""
    x = music_rows(LONG_T_IN, LONG_SEEDS)
    x.setflags(write=False)
    T_out = [int(np.floor(LONG_T_IN / float(r))) for r in LONG_RATIOS]
    return x, T_out, [stretch_f64(row, float(r), t, 0) for row, r, t in zip(x, LONG_RATIOS, T_out)]


@functools.lru_cache(maxsize=None)
def tie_case():
    """Case 2: one integer row of period 64 at 0.94 and 1.06, no read in the padding
    -> (x, x_offset, T_out, [Stretch at 0.94, Stretch at 1.06])."""
    from grafp_amd import ops
    pad, T_in = ops.stretch_pad(1.06), ops.stretch_input_len(T_SMALL, 1.06)
    x = tie_row(T_in, 5)
    x.setflags(write=False)
    return x, pad, T_SMALL, [stretch_f64(x, float(F32(r)), T_SMALL, pad) for r in (0.94, 1.06)]


def tie_row(T, seed):
    """(T,) f32 of integers in [-7, 7] with period 64: every correlation is an integer below 2^24, exact in f32 in any
    order, and candidates 64 apart tie exactly wherever no read touches the padding."""
    return np.tile(np.random.default_rng(seed).integers(-7, 8, 64), -(-T // 64))[:T].astype(F32)
