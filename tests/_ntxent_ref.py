"""Float64 reference of NT-Xent (grafp_amd/csrc/ntxent.hip), its input builders, bars and the table of cases that
tests/test_ntxent_cpu.py and tests/test_gpu_ntxent.py run (TEST INFRASTRUCTURE).  Plain numpy: nothing here is imported
from grafp_amd or torch.

Definitions (those at the top of ntxent.hip): rows are ordered [view i | view j], M = 2 B of them; S = z z^T / tau;
partner(r) = r + B for r < B, r - B otherwise; lse[r] = log sum_{c != r} exp S[r][c]; pos[r] = S[r][partner(r)];
loss = mean_r (lse[r] - pos[r]).  With P[r][c] = exp(S[r][c] - lse[r]) (0 on the diagonal) and Y the partner one-hot,
dz = (W + W^T) z / tau, W = (P - Y) / M.

Bars (f32 kernels against float64).  nmax = the largest row norm, Lmax = nmax^2 / tau + ln(2B) bounds |lse| and |pos|,
G0 = nmax / (tau 2B) is what one unit softmax weight adds to a gradient entry.
  per row lse - pos   |err| <= 2e-5 |value| + 8 * 2^-23 * Lmax      (the project's loss bar + lse and pos each stored as
                                                                     one f32 of magnitude up to Lmax)
  loss                the same; a loss partial: the sum of the bars of its rows (lse - pos >= 0, so the sum of the row
                      bars over all rows, divided by 2B, IS the loss bar)
  gradients           |err| <= 1e-4 |want| + 1e-5 G0"""
import collections
import functools

import numpy as np

from _hashfill import hash_normalish

NT_Q, NT_C = 32, 128                      # query rows per workgroup / candidate rows per chunk (ntxent.hip)
LOSS_RTOL, GRAD_RTOL, GRAD_G0 = 2e-5, 1e-4, 1e-5
F32_ULPS = 8.0 * 2.0 ** -23

# ---- the cases ------------------------------------------------------------------------------------------------------
Full = collections.namedtuple("Full", "B D tau kind")
Local = collections.namedtuple("Local", "B D tau kind row_begin n_local")

FULL_CASES = [
    Full(1, 32, 0.05, "unit"),            # the degenerate case: loss exactly 0, gradients exactly 0
    Full(2, 96, 0.05, "unit"),
    Full(33, 96, 0.1, "unit"),
    Full(129, 64, 0.05, "unit"),          # 3 chunks (2-row tail), one split
    Full(193, 128, 0.05, "unit"),         # 4 chunks (2-row tail), 2 x 2
    Full(300, 64, 0.05, "norms"),         # 5 chunks dealt 3 + 2
    Full(520, 128, 0.05, "unit"),         # 9 chunks, 4 x 3: the last split is empty in both passes
    Full(577, 32, 0.05, "unit"),          # 10 chunks (2-row tail), 5 x 2
    Full(1100, 64, 0.05, "unit"),         # 18 chunks, 8 x 3: two empty splits; pass 2 has 3 x 6
    Full(2049, 32, 0.5, "unit"),          # 33 chunks, 8 x 5: one empty split; pass 2 unsplit
    Full(100, 128, 0.01, "unit"),         # logits up to 100, softmax near one-hot
    Full(70, 64, 0.05, "dup"),
    Full(193, 128, 0.05, "dup"),
    Full(193, 64, 0.1, "norms"),
]
LOCAL_CASES = [
    Local(193, 128, 0.05, "unit", 17, 50),
    Local(520, 128, 0.05, "unit", 455, 65),      # the range ends at B_all
    Local(520, 128, 0.05, "unit", 3, 7),
    Local(1100, 64, 0.05, "unit", 963, 137),
    Local(33, 128, 0.05, "unit", 32, 1),
]
PARTITION_520 = [(0, 3), (3, 7), (10, 190), (200, 255), (455, 65)]      # ragged parts of [0, 520), D = 128, tau 0.05


def case_id(c):
    s = f"{c.B}-{c.D}-{c.tau}-{c.kind}"
    return s if isinstance(c, Full) else f"{s}-{c.row_begin}+{c.n_local}"


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _unit(B, D):
    """Unit-norm rows, built the way test_ntxent_vs_oracle builds them."""
    zi = hash_normalish(f"nt64:zi.{B}.{D}", (B, D))
    zj = zi + 2.0 * hash_normalish(f"nt64:zj.{B}.{D}", (B, D))
    zi /= np.linalg.norm(zi, axis=1, keepdims=True)
    zj /= np.linalg.norm(zj, axis=1, keepdims=True)
    return zi.astype(np.float32), zj.astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(B, D, kind):
    """(zi, zj) float32 (B, D), read-only.
    unit   unit-norm rows
    dup    zj = zi exactly and, for B > 3, row 3 a copy of row 1 in both views: the positives sit at the maximum logit and
           there are exact ties among the negatives
    norms  row norms spread geometrically over [e^-0.7, e^0.7], in opposite order in the two views"""
    zi, zj = _unit(B, D)
    if kind == "dup":
        if B > 3:
            zi[3] = zi[1]
        zj = zi.copy()
    elif kind == "norms":
        g = np.exp(np.linspace(-0.7, 0.7, B))[:, None]
        zi = (zi * g).astype(np.float32)
        zj = (zj * g[::-1]).astype(np.float32)
    else:
        assert kind == "unit", kind
    zi.setflags(write=False)
    zj.setflags(write=False)
    return zi, zj


# ---- the reference --------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "loss lse pos dzi dzj")
LocalRef = collections.namedtuple("LocalRef", "share dzi dzj partials")


def ntxent_f64(zi, zj, tau):
    """(loss, lse (2B,), pos (2B,), dzi (B, D), dzj (B, D)) in float64.  A NaN input propagates as IEEE arithmetic has it."""
    z = np.concatenate([np.asarray(zi, np.float64), np.asarray(zj, np.float64)], axis=0)
    B, M = zi.shape[0], 2 * zi.shape[0]
    partner = (np.arange(M) + B) % M
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        S = (z @ z.T) / float(tau)
        np.fill_diagonal(S, -np.inf)
        m = S.max(axis=1)                                              # np.max propagates NaN
        P = np.exp(S - m[:, None])
        lse = m + np.log(P.sum(axis=1))
        pos = S[np.arange(M), partner]
        P /= P.sum(axis=1, keepdims=True)
        P[np.arange(M), partner] -= 1.0
        P += P.T.copy()
        dz = (P @ z) / (float(tau) * M)
        loss = float(np.mean(lse - pos))
    return Ref(loss, lse, pos, dz[:B], dz[B:])


def local_f64(ref, row_begin, n_local):
    """The range's share of the global mean loss, the global gradient restricted to the local rows, and the sums of
    lse - pos per (view, 32-row block) -- the order of loss_partial."""
    B = ref.dzi.shape[0]
    v = ref.lse - ref.pos
    lo, hi = row_begin, row_begin + n_local
    parts = [v[view * B + b0:view * B + min(b0 + NT_Q, hi)].sum() for view in (0, 1) for b0 in range(lo, hi, NT_Q)]
    share = float((v[lo:hi].sum() + v[B + lo:B + hi].sum()) / (2 * B))
    return LocalRef(share, ref.dzi[lo:hi], ref.dzj[lo:hi], np.asarray(parts, np.float64))


@functools.lru_cache(maxsize=None)
def cached_ref(B, D, tau, kind):
    """The float64 reference of a case's inputs, computed once per session and shared (read-only)."""
    zi, zj = inputs(B, D, kind)
    ref = ntxent_f64(zi, zj, tau)
    for a in ref[1:]:
        a.setflags(write=False)
    return ref


# ---- bars -----------------------------------------------------------------------------------------------------------
Bars = collections.namedtuple("Bars", "nmax Lmax G0")


def scales(zi, zj, tau):
    with np.errstate(invalid="ignore"):
        n = np.concatenate([np.linalg.norm(np.asarray(zi, np.float64), axis=1), np.linalg.norm(np.asarray(zj, np.float64), axis=1)])
    nmax = float(np.nanmax(n))
    M = 2 * zi.shape[0]
    return Bars(nmax, nmax * nmax / tau + np.log(M), nmax / (tau * M))


def row_bars(ref, sc):
    """Bar of lse[r] - pos[r] per row, (2B,)."""
    return LOSS_RTOL * np.abs(ref.lse - ref.pos) + F32_ULPS * sc.Lmax


def loss_bar(loss, sc):
    return LOSS_RTOL * abs(loss) + F32_ULPS * sc.Lmax


def partial_bars(ref, sc, row_begin, n_local):
    """Bars of the loss partials (the sum of the bars of each partial's rows), in the order of loss_partial."""
    B = ref.dzi.shape[0]
    rb = row_bars(ref, sc)
    lo, hi = row_begin, row_begin + n_local
    return np.asarray([rb[view * B + b0:view * B + min(b0 + NT_Q, hi)].sum() for view in (0, 1) for b0 in range(lo, hi, NT_Q)])


def grad_bar(want, sc):
    return GRAD_RTOL * np.abs(want) + GRAD_G0 * sc.G0


def worst(got, want, bar):
    """max |got - want| / bar (<= 1 passes); a non-finite difference counts as infinitely bad."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / bar
    d = np.where(np.isfinite(d), d, np.inf)
    return float(np.max(d)) if d.size else 0.0


# ---- the launch plan, as grafp_ntxent_plan reports it -----------------------------------------------------------------
Plan = collections.namedtuple("Plan", "chunks splits rows splits2 rows2 partials")


def plan(lib, B_all, n_local):
    import ctypes
    info = (ctypes.c_int * 8)()
    assert lib.grafp_ntxent_plan(B_all, n_local, info) == 0, lib.grafp_last_error()
    assert list(info[6:8]) == [0, 0]
    return Plan(*info[:6])


def empty_splits(chunks, splits, rows):
    """Trailing splits whose candidate range [s * rows, ...) starts at or past the last chunk."""
    per = rows // NT_C
    return splits - (chunks + per - 1) // per


def plan_bytes(p, B_all, n_local, D):
    """Bytes a call uses of its workspace, in the layout ntxent.hip states: lse[M] | pos[M] | pass-1 triples
    [splits][M][3] | pass-2 partial gradients [splits2][2][n_local][D]."""
    M = 2 * B_all
    return 4 * (2 * M + p.splits * M * 3 + p.splits2 * 2 * n_local * D)
