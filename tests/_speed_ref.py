"""CPU restatements of grafp_speed_change_f32 (csrc/speed.hip) for tests/test_speed_cpu.py, tests/test_gpu_speed.py and
tools/speed_bench.py: the rule in float64, and the kernel's own route in numpy float32, operation by operation."""
import math

import numpy as np

F = np.float32
PI = F(3.14159265358979323846)           # SP_PI
PI_12 = F(0.26179938779914943654)        # SP_PI_12
WMAX = 13                                 # SP_WMAX


def clamp_ratio(r):
    """The kernels' warp_ratio (csrc/clipwarp.h) on an f32: NaN -> 1, then [0.5, 2]."""
    r = F(r)
    if r != r:
        return F(1.0)
    return F(0.5) if r < F(0.5) else (F(2.0) if r > F(2.0) else r)


def _padded(x, lo, hi, dtype):
    """xz[lo .. hi] (x inside [0, len), 0 outside) -> (array, index of xz[0] in it)."""
    x = np.asarray(x, dtype=dtype)
    lo, hi = min(int(lo), 0), max(int(hi), x.size - 1)
    buf = np.zeros(hi - lo + 1, dtype=dtype)
    buf[-lo:-lo + x.size] = x
    return buf, -lo


def tap_range(p, rho):
    """First and last k of the rule's sum at position(s) p: ceil(p - 6/c), floor(p + 6/c)."""
    reach = 6.0 / (0.99 * min(1.0, 1.0 / rho))
    return np.ceil(p - reach).astype(np.int64), np.floor(p + reach).astype(np.int64)


def speed_f64(x, rho, out_len, x_offset=0, m_from=0, copy_at_one=True):
    """The rule in float64 for one clip: outputs m_from .. out_len - 1.  rho: a float, used as given after the clamp (the
    GPU tests pass the f32 ratio's value).  copy_at_one=False evaluates the filter at rho == 1 too instead of the rule's
    copy: that is what a polyphase resampler between equal rates computes (the 0.99 roll-off is not the identity)."""
    rho = float(rho)
    rho = 1.0 if rho != rho else min(max(rho, 0.5), 2.0)
    m = np.arange(m_from, out_len, dtype=np.float64)
    p = float(x_offset) + m * rho
    copy = rho == 1.0 and copy_at_one
    if copy:
        klo = khi = p.astype(np.int64)
    else:
        klo, khi = tap_range(p, rho)
    xz, z = _padded(x, klo.min(), khi.max(), np.float64)
    if copy:
        return xz[klo + z]
    c = 0.99 * min(1.0, 1.0 / rho)
    out = np.zeros(m.size)
    for j in range(int((khi - klo).max()) + 1):
        k = np.minimum(klo + j, khi)
        t = np.clip(c * (k - p), -6.0, 6.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(t == 0, 1.0, np.sin(math.pi * t) / (math.pi * t))
        h = c * sinc * np.cos(math.pi * t / 12.0) ** 2
        out += np.where(klo + j <= khi, xz[k + z] * h, 0.0)
    return out


def _fma(a, b, c):
    """fmaf on f32 arrays: the product of two f32 is exact in f64; the sum is rounded to f64, then to f32 (differs from
    one rounding in about one case in 2^29)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def speed_f32(x, rho, out_len, x_offset=0, m_from=0):
    """speed_change_kernel's route in numpy f32, operation by operation: p in f64 from the f32 rho, split into floor(p)
    and f = (float)(p - floor(p)); per candidate j = -W .. W + 1: t = c * ((float)j - f), used iff |t| <= 6;
    sin(pi t) = (-1)^n sinf(pi * (t - n)) with n = rintf(t); sinc = that / (pi * t) (1 at 0); w = cosf(t * pi/12);
    h = ((c * sinc) * w) * w; acc = fmaf(x, h, acc)."""
    rho = clamp_ratio(rho)
    m = np.arange(m_from, out_len, dtype=np.float64)
    p = np.float64(x_offset) + m * np.float64(rho)
    fl = np.floor(p)
    ip = fl.astype(np.int64)
    if rho == F(1.0):
        xz, z = _padded(x, ip.min(), ip.max(), F)
        return xz[ip + z]
    f = (p - fl).astype(F)
    c = F(0.99) * min(F(1.0), F(1.0) / rho)
    W = min(WMAX, int(F(6.0) / c + F(1e-3)))
    xz, z = _padded(x, ip.min() - W, ip.max() + W + 1, F)
    acc = np.zeros(m.size, dtype=F)
    for j in range(-W, W + 2):
        t = c * (F(j) - f)
        n = np.rint(t)
        s = np.sin(PI * (t - n))
        s = np.where(n.astype(np.int64) & 1, -s, s)
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(t == 0, F(1.0), s / (PI * t))
        cw = np.cos(t * PI_12)
        h = c * sinc * cw * cw
        assert h.dtype == F and t.dtype == F
        acc = np.where(np.abs(t) <= F(6.0), _fma(xz[ip + j + z], h, acc), acc)
    return acc


# ---- case generators ---------------------------------------------------------------------------------------------
SMALL_RATIOS = np.array([0.5, 0.94, 1.0, np.nextafter(F(1.0), F(2.0)), 1.06, 2.0], dtype=F)


def uniform_rows(B, T, seed):
    """(B, T) f32 uniform in [-1, 1]."""
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=(B, T)).astype(F)


def batch_refs(x, ratios, out_len, x_offset=0, m_from=0):
    """(speed_f64, speed_f32) of every row of x at its ratio -> two (B, out_len - m_from) arrays."""
    r64 = np.stack([speed_f64(row, float(clamp_ratio(r)), out_len, x_offset, m_from) for row, r in zip(x, ratios)])
    r32 = np.stack([speed_f32(row, r, out_len, x_offset, m_from) for row, r in zip(x, ratios)])
    return r64, r32
