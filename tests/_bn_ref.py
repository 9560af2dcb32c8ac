"""Float64 reference of the fused [pre-bias] + BatchNorm + activation + residual (grafp_amd/csrc/bn.hip) and the table of
cases tests/test_bn_cpu.py and tests/test_gpu_bn.py run (TEST INFRASTRUCTURE).  Plain formulas in numpy: nothing here is
imported from grafp_amd and nothing calls torch's batch_norm (test_bn_cpu.py pins these formulas against it).

Conventions: x, dz, residual (C, M) rows; a row is G views of Mg = M / G columns with their own batch statistics; the
running statistics advance once per view, in view order.  The derivative of the activation is the negative-side slope
wherever the pre-activation is not > 0, a NaN pre-activation included (what torch's leaky_relu_backward does) -- NaN
reaches dx through xhat, not through the mask."""
import collections
import functools

import numpy as np

from _hashfill import hash_normalish, hash_uniform

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.2
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
PATH_1PASS, PATH_2PASS_VEC, PATH_2PASS_SCALAR = 0, 1, 2

# f32 bars (those of test_bn_act_forward_backward_f32)
OUT_RTOL = OUT_ATOL = 2e-5
GRAD_RTOL = 1e-4
LONG_ROW = 1 << 16          # columns per view from which the bars come from long_row_error instead
LONG_ROW_FACTOR = 16.0
BF16_ULP = 2.0 ** -8

# fwd / bwd: the launch grafp_bn_plan must report = (path, vectors per thread, threads, chunks per view), worked out by hand
# from the rules in bn.hip (W = 4 f32 / 8 bf16 elements per 16-byte vector):
#   single-pass forward   chunk = 256 * 8 * W                       (f32 8192, bf16 16384)
#   single-pass backward  f32 256 * 4 * 4 = 4096;  bf16 256 * 4 * 8 = 8192, above 16 chunks per row 256 * 8 * 8 = 16384,
#                         and from 32 such chunks per view 512 * 8 * 8 = 32768;  more than 256 chunks per row: two-pass
#   two-pass              S = min(ceil(Mg / (1024 W')), max(4096 / (C G), 1)), chunk = ceil(Mg / S) rounded up to W',
#                         chunks = ceil(Mg / chunk); W' = W on the vector path, 1 on the scalar path
# misalign: None, or which operand ("x", "dz", "res") is a contiguous view at storage offset 1 of a larger buffer.
Case = collections.namedtuple("Case", "name dt C Mg G act pb res training two_pass misalign fwd bwd")

_1P, _2V, _2S = PATH_1PASS, PATH_2PASS_VEC, PATH_2PASS_SCALAR
CASES = [
    # ---- single pass, f32: one backward chunk; 3 * 4096 + 4 = four backward / two forward chunks, the last of 4 elements
    Case("f32-1p-4096", "f32", 3, 4096, 1, ACT_RELU, True, False, True, False, None, (_1P, 8, 256, 1), (_1P, 4, 256, 1)),
    Case("f32-1p-ragged", "f32", 3, 12292, 1, ACT_LEAKY, False, True, True, False, None, (_1P, 8, 256, 2), (_1P, 4, 256, 4)),
    Case("f32-1p-ragged-2v", "f32", 2, 12292, 2, ACT_NONE, True, True, True, False, None, (_1P, 8, 256, 2), (_1P, 4, 256, 4)),
    Case("f32-1p-4096-3v", "f32", 3, 4096, 3, ACT_RELU, False, False, True, False, None, (_1P, 8, 256, 1), (_1P, 4, 256, 1)),
    # ---- single pass, bf16: 4 vectors / 256 threads, 8 / 256, 8 / 512
    Case("bf16-1p-i4", "bf16", 3, 16392, 1, ACT_RELU, True, True, True, False, None, (_1P, 8, 256, 2), (_1P, 4, 256, 3)),
    Case("bf16-1p-i4-2v", "bf16", 2, 16392, 2, ACT_LEAKY, False, False, True, False, None, (_1P, 8, 256, 2), (_1P, 4, 256, 3)),
    Case("bf16-1p-i8", "bf16", 2, 17 * 8192, 1, ACT_NONE, True, False, True, False, None, (_1P, 8, 256, 9), (_1P, 8, 256, 9)),
    Case("bf16-1p-i8-t512-2v", "bf16", 2, 31 * 16384 + 8, 2, ACT_RELU, False, True, True, False, None,
         (_1P, 8, 256, 32), (_1P, 8, 512, 16)),
    # ---- more than 256 chunks per row: falls back to the two-pass kernels by itself
    Case("f32-over256", "f32", 2, 257 * 8192, 1, ACT_LEAKY, True, False, True, False, None, (_2V, 0, 256, 514), (_2V, 0, 256, 514)),
    Case("bf16-over256", "bf16", 2, 257 * 32768, 1, ACT_RELU, False, True, True, False, None,
         (_2V, 0, 256, 1028), (_2V, 0, 256, 1028)),
    # ---- two-pass on vectors: by the switch and by eval mode; several chunks, and C = 2048 where one chunk is left
    Case("f32-2p-switch-2v", "f32", 3, 5 * 4096 + 4, 2, ACT_RELU, True, True, True, True, None, (_2V, 0, 256, 6), (_2V, 0, 256, 6)),
    Case("bf16-2p-switch", "bf16", 3, 5 * 4096 + 8, 1, ACT_LEAKY, False, False, True, True, None, (_2V, 0, 256, 3), (_2V, 0, 256, 3)),
    Case("f32-2p-eval", "f32", 2, 5 * 4096 + 4, 1, ACT_NONE, True, False, False, False, None, (_2V, 0, 256, 6), (_2V, 0, 256, 6)),
    Case("bf16-2p-eval-2v", "bf16", 2, 5 * 4096 + 8, 2, ACT_RELU, True, True, False, False, None, (_2V, 0, 256, 3), (_2V, 0, 256, 3)),
    Case("f32-2p-wide", "f32", 2048, 256, 1, ACT_RELU, False, False, True, True, None, (_2V, 0, 256, 1), (_2V, 0, 256, 1)),
    Case("bf16-2p-wide", "bf16", 2048, 256, 1, ACT_LEAKY, True, False, True, True, None, (_2V, 0, 256, 1), (_2V, 0, 256, 1)),
    # ---- two-pass scalar: rows that are no whole vectors ...
    Case("f32-sc-1001", "f32", 3, 1001, 1, ACT_RELU, True, True, True, False, None, (_2S, 0, 256, 1), (_2S, 0, 256, 1)),
    Case("bf16-sc-1001", "bf16", 3, 1001, 1, ACT_LEAKY, False, False, True, False, None, (_2S, 0, 256, 1), (_2S, 0, 256, 1)),
    Case("f32-sc-1001-3v", "f32", 2, 1001, 3, ACT_NONE, True, True, True, False, None, (_2S, 0, 256, 1), (_2S, 0, 256, 1)),
    Case("bf16-sc-1001-3v", "bf16", 2, 1001, 3, ACT_RELU, True, False, True, False, None, (_2S, 0, 256, 1), (_2S, 0, 256, 1)),
    Case("f32-sc-7", "f32", 3, 7, 1, ACT_LEAKY, False, True, True, False, None, (_2S, 0, 256, 1), (_2S, 0, 256, 1)),
    Case("bf16-sc-7", "bf16", 3, 7, 1, ACT_RELU, True, True, True, False, None, (_2S, 0, 256, 1), (_2S, 0, 256, 1)),
    # ---- ... and whole vectors at a base pointer one element off: the launch that gets the misaligned pointer goes scalar
    # (4 chunks of 1024), the other one stays on the single pass
    Case("f32-off1-x", "f32", 2, 4096, 1, ACT_RELU, True, True, True, False, "x", (_2S, 0, 256, 4), (_2S, 0, 256, 4)),
    Case("f32-off1-dz", "f32", 2, 4096, 1, ACT_LEAKY, False, True, True, False, "dz", (_1P, 8, 256, 1), (_2S, 0, 256, 4)),
    Case("f32-off1-res", "f32", 2, 4096, 1, ACT_NONE, True, True, True, False, "res", (_2S, 0, 256, 4), (_1P, 4, 256, 1)),
    Case("bf16-off1-x-2v", "bf16", 2, 4096, 2, ACT_LEAKY, True, True, True, False, "x", (_2S, 0, 256, 4), (_2S, 0, 256, 4)),
    Case("bf16-off1-dz", "bf16", 2, 4096, 1, ACT_RELU, False, True, True, False, "dz", (_1P, 8, 256, 1), (_2S, 0, 256, 4)),
    Case("bf16-off1-res", "bf16", 2, 4096, 1, ACT_NONE, True, True, True, False, "res", (_2S, 0, 256, 4), (_1P, 4, 256, 1)),
    # ---- eval mode on the remaining dtype x views combinations (with pre_bias)
    Case("f32-eval-sc-2v", "f32", 3, 1001, 2, ACT_LEAKY, True, True, False, False, None, (_2S, 0, 256, 1), (_2S, 0, 256, 1)),
    Case("bf16-eval", "bf16", 3, 4096, 1, ACT_NONE, True, False, False, False, None, (_2V, 0, 256, 1), (_2V, 0, 256, 1)),
]
CASE_BY_NAME = {c.name: c for c in CASES}
SMALL_CASES = [c.name for c in CASES if c.C * c.Mg * c.G <= 1 << 17]        # the ones pinned against torch on the CPU


def bf16_round(a):
    """float32 array -> nearest-even bfloat16, widened back to float32 (finite values)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def _fill(name, shape):
    # bell-shaped where a test can afford four hashes per element, uniform with unit variance above a million elements
    if int(np.prod(shape)) > 1 << 20:
        return hash_uniform(name, shape) * np.float32(np.sqrt(3.0))
    return hash_normalish(name, shape)


def case_inputs(case):
    """float32 arrays (bf16 cases: already rounded to bf16 values) -- x, dz, res (or None), gamma, beta, pb (or None), rm0,
    rv0.  Row 0 has |mean| = 30 std (std 2), row 1 std 6, row 2 (where there is one) is constant at 3.0; further rows std 2
    and means up to 15 std."""
    c, n = case, case.name
    M = c.Mg * c.G
    std = np.full((c.C, 1), 2.0, np.float32)
    std[1::3] = 6.0
    mu = 15.0 * hash_uniform(f"bn:{n}.mu", (c.C, 1))
    mu[0] = 30.0
    mu[1] = 0.25
    x = (_fill(f"bn:{n}.x", (c.C, M)) + mu) * std
    if c.C >= 3:
        x[2] = 3.0
    dz = _fill(f"bn:{n}.dz", (c.C, M))
    res = _fill(f"bn:{n}.res", (c.C, M)) if c.res else None
    if c.dt == "bf16":
        x, dz = bf16_round(x), bf16_round(dz)
        res = bf16_round(res) if c.res else None
    gamma = 1.0 + 0.2 * hash_uniform(f"bn:{n}.g", (c.C,))
    beta = 0.3 * hash_uniform(f"bn:{n}.b", (c.C,))
    pb = 0.5 * hash_uniform(f"bn:{n}.pb", (c.C,)) if c.pb else None
    rm0 = 0.1 * hash_uniform(f"bn:{n}.rm", (c.C,))
    rv0 = 1.0 + 0.5 * np.abs(hash_uniform(f"bn:{n}.rv", (c.C,)))
    return dict(x=x, dz=dz, res=res, gamma=gamma, beta=beta, pb=pb, rm0=rm0, rv0=rv0)


def bn_ref(x, dz, res, gamma, beta, pb, rm0, rv0, G, act, training, slope=SLOPE, eps=EPS, momentum=MOMENTUM,
           dtype=np.float64, side=None):
    """The whole forward and backward in `dtype` (float64: the reference; float32: the same formulas, to measure what
    f32 arithmetic costs on long rows -- there `side` hands in the reference's pre-activation > 0 decisions, so that the
    measurement holds no flipped ReLU side).  Returns a dict: out, pre (the pre-activation), mean, invstd (C, G), rm, rv, dx,
    dgamma, dbeta, dpb, dres, xhat, dy, dz."""
    f = lambda a: None if a is None else np.asarray(a, dtype=dtype)          # noqa: E731
    x, dz, res, gamma, beta, pb, rm0, rv0 = map(f, (x, dz, res, gamma, beta, pb, rm0, rv0))
    C, M = x.shape
    Mg = M // G
    one = dtype(1.0)
    xv = x.reshape(C, G, Mg)
    if pb is not None:
        xv = xv + pb[:, None, None]
    rm, rv = rm0.copy(), rv0.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if training:
            mean = xv.mean(axis=2, dtype=dtype)
            var = np.square(xv - mean[:, :, None]).mean(axis=2, dtype=dtype)            # biased: normalisation
            unbiased = var * dtype(Mg / (Mg - 1.0)) if Mg > 1 else var                # unbiased: running update
            for g in range(G):                                                         # once per view, in view order
                rm = (one - dtype(momentum)) * rm + dtype(momentum) * mean[:, g]
                rv = (one - dtype(momentum)) * rv + dtype(momentum) * unbiased[:, g]
        else:
            mean = np.repeat(rm0[:, None], G, axis=1)
            var = np.repeat(rv0[:, None], G, axis=1)
        invstd = one / np.sqrt(var + dtype(eps))
        xh = (xv - mean[:, :, None]) * invstd[:, :, None]
        del xv
        pre = xh * gamma[:, None, None] + beta[:, None, None]
        side = pre > 0 if side is None else np.asarray(side).reshape(pre.shape)
        neg = one if act == ACT_NONE else (dtype(0.0) if act == ACT_RELU else dtype(slope))
        if act == ACT_NONE:
            out = pre.copy()
        elif act == ACT_RELU:
            out = np.maximum(pre, dtype(0.0))                                           # keeps NaN, as torch.relu does
        else:
            out = np.where(side, pre, pre * dtype(slope))
        if res is not None:
            out = out + res.reshape(C, G, Mg)
        dy = dz.reshape(C, G, Mg) * np.where(side, one, neg)
        dyx = dy * xh
        dbeta = dy.sum(axis=(1, 2), dtype=dtype)
        dgamma = dyx.sum(axis=(1, 2), dtype=dtype)
        k = (gamma[:, None] * invstd)[:, :, None]
        if training:
            dx = k * (dy - dy.mean(axis=2, dtype=dtype)[:, :, None] - xh * dyx.mean(axis=2, dtype=dtype)[:, :, None])
            dpb = np.zeros(C, dtype)                                                    # cancels under batch statistics
        else:
            dx = k * dy
            dpb = (gamma[:, None] * invstd * dy.sum(axis=2, dtype=dtype)).sum(axis=1)
        del dyx
    return dict(out=out.reshape(C, M), pre=pre.reshape(C, M), mean=mean, invstd=invstd, rm=rm, rv=rv, dx=dx.reshape(C, M),
                dgamma=dgamma, dbeta=dbeta, dpb=dpb if pb is not None else None, dres=dz if res is not None else None,
                xhat=xh.reshape(C, M), dy=dy.reshape(C, M), dz=dz)


def case_ref(case, dtype=np.float64, inputs=None, side=None):
    i = inputs if inputs is not None else case_inputs(case)
    return bn_ref(i["x"], i["dz"], i["res"], i["gamma"], i["beta"], i["pb"], i["rm0"], i["rv0"], case.G, case.act,
                  case.training, dtype=dtype, side=side)


@functools.lru_cache(maxsize=2)
def cached_case(name):
    """(inputs, float64 reference) of a case, computed once and shared; callers must not write into either."""
    case = CASE_BY_NAME[name]
    inputs = case_inputs(case)
    return inputs, case_ref(case, inputs=inputs)


def ambiguous(case, ref):
    """Positions whose ReLU / LeakyReLU side an f32 kernel may legitimately decide the other way: the float64
    pre-activation lies within the f32 output bar of zero.  (No activation: none.)"""
    if case.act == ACT_NONE:
        return np.zeros(ref["pre"].shape, bool)
    return np.abs(ref["pre"]) <= OUT_ATOL + OUT_RTOL * np.abs(ref["pre"])


def long_row_error(case, inputs, ref):
    """Rows of 2^16 columns per view and more: max |float32 formulas - float64 formulas| per result on the case's own
    inputs (numpy float32 throughout, pairwise sums), or None for shorter rows.  The GPU test allows LONG_ROW_FACTOR times
    this where that is more than the f32 bar."""
    if case.Mg < LONG_ROW:
        return None
    r32 = case_ref(case, dtype=np.float32, inputs=inputs, side=ref["pre"] > 0)
    err = {}
    for key in ("out", "mean", "invstd", "rm", "rv", "dx", "dgamma", "dbeta"):
        err[key] = float(np.max(np.abs(r32[key].astype(np.float64) - ref[key])))
    return err


def bars(case, ref, long_err=None):
    """Per result the elementwise bound on |got - ref| (arrays or scalars), from the f32 bars of
    test_bn_act_forward_backward_f32, one bf16 rounding for bf16 out / dx, the ambiguous ReLU positions' share of dgamma
    and dbeta, and, on long rows, 16 x the measured float32 error where that is larger."""
    amb = ambiguous(case, ref)
    half = BF16_ULP if case.dt == "bf16" else 0.0
    gmax = lambda a: float(np.max(np.abs(a)))            # noqa: E731
    dz_amb = np.abs(np.where(amb, ref["dz"], 0.0))
    b = {
        "out": OUT_ATOL + (OUT_RTOL + half) * np.abs(ref["out"]),
        "dx": GRAD_RTOL * gmax(ref["dx"]) + (GRAD_RTOL + half) * np.abs(ref["dx"]),
        "dgamma": GRAD_RTOL * gmax(ref["dgamma"]) + 1e-7 + GRAD_RTOL * np.abs(ref["dgamma"]),
        "dbeta": GRAD_RTOL * gmax(ref["dbeta"]) + 1e-7 + GRAD_RTOL * np.abs(ref["dbeta"]),
        "mean": 1e-5 + 1e-5 * np.abs(ref["mean"]),
        "invstd": 1e-5 + 1e-4 * np.abs(ref["invstd"]),
        "rm": 1e-5 + 1e-5 * np.abs(ref["rm"]),
        "rv": 1e-5 + 1e-4 * np.abs(ref["rv"]),
    }
    b["dbeta"] = b["dbeta"] + dz_amb.sum(axis=1)
    b["dgamma"] = b["dgamma"] + (dz_amb * np.abs(ref["xhat"])).sum(axis=1)
    if long_err is not None:
        for key, e in long_err.items():
            b[key] = np.maximum(b[key], LONG_ROW_FACTOR * e)
    return b, amb
