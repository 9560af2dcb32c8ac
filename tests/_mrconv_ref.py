"""Reference and case table of the max-relative tests (TEST INFRASTRUCTURE): tests/test_mrconv_cpu.py pins them on the
CPU, tests/test_gpu_mrconv.py compares every launch path of grafp_amd/csrc/mrconv.hip with them, exactly.

Exact, because the inputs make the exact result representable:
  * forward: one subtraction and a maximum -- exact for any x; here x = round(4 hash_normalish) / 4, plus 1/4 per group of
    16 clips (|x| < 8: five bits, held exactly by bf16), which also gives many ties among a node's neighbours (first
    maximum wins);
  * backward: gradients are multiples of 2^-4 with |g| <= 3 (bf16 holds them).  The kernels scatter in fixed point with
    the scale 2^37 of a largest addend in [2, 4), so every addend is an integer there; a node receives at most N of them,
    so every partial sum is at most 3 N <= 12 300 < 2^15 and, as a multiple of 2^-4, exact in f32 (19 + 4 bits), as is
    base + sum with |base| <= 6.  The f32 result is therefore the exact one and the bf16 result the exact one rounded once.
The paths of the table were worked out by hand from the host code; grafp_mrconv_plan must report them."""
import functools
from collections import namedtuple

import numpy as np

from _hashfill import hash_ints, hash_normalish

PERSISTENT, VEC4, SCALAR, RECORD = 0, 1, 2, 3
G_MAX, G_STEP = 3.0, 1.0 / 16.0

# fwd / bwd: (path, items per thread, channel rows per slab, slabs per clip, workgroups per clip) of the call that records
# nothing (ops.switches.mrconv_arg off, or a shape without a record); rec: the same pair for the recording call, None where
# the shape has no record.  off1: x is a contiguous view at storage offset 1 (a misaligned pointer).
Case = namedtuple("Case", "name B C N K idx32 off1 fwd bwd rec")
CASES = [
    # persistent, one slab per workgroup (B = 2: per_clip grows to the slab count), short last slab: 10 = 4 + 4 + 2 / 2 x 5
    Case("persistent-short-last", 2, 10, 1000, 3, False, False, (PERSISTENT, 4, 4, 3, 3), (PERSISTENT, 2, 2, 5, 5),
         ((RECORD, 4, 4, 3, 3), (RECORD, 2, 2, 5, 5))),
    # persistent, 4 workgroups per clip (4 x 256 = 1024): forward 18 slabs of 64 rows (the last 12), 5 for workgroup 0 and
    # 4 / 2 register sets; backward 35 slabs of 32 rows (the last 12): the pipelines are refilled
    Case("persistent-refill", 256, 1100, 64, 3, True, False, (PERSISTENT, 4, 64, 18, 4), (PERSISTENT, 2, 32, 35, 4),
         ((RECORD, 4, 64, 18, 4), (RECORD, 2, 32, 35, 4))),
    # N > 4096: no persistent kernel; 4-wide generic, one row per slab, backward with 8 pieces per thread
    Case("vec4-items8", 1, 3, 4100, 2, False, False, (VEC4, 0, 1, 3, 3), (VEC4, 8, 1, 3, 3), None),
    # K N = 35 840 > 34 816: the persistent backward's LDS does not fit, the generic one's does with one row per slab
    Case("vec4-items2", 1, 3, 1024, 35, False, False, (PERSISTENT, 4, 3, 1, 1), (VEC4, 2, 1, 3, 3), None),
    # N % 4 != 0: scalar; 4096 / 1001 = 4 rows forward, 2048 / 1001 = 2 rows backward
    Case("scalar-items8", 2, 5, 1001, 3, False, False, (SCALAR, 0, 4, 2, 2), (SCALAR, 8, 2, 3, 3), None),
    Case("scalar-items2", 2, 10, 101, 3, False, False, (SCALAR, 0, 10, 1, 1), (SCALAR, 2, 5, 2, 2), None),
    # aligned shape, misaligned pointer: scalar although x requires a gradient and the shape has a record
    Case("scalar-by-pointer", 2, 8, 64, 3, False, True, (SCALAR, 0, 8, 1, 1), (SCALAR, 2, 8, 1, 1), None),
]
CASE_BY_NAME = {c.name: c for c in CASES}
SMALL_CASES = [c.name for c in CASES if c.B * c.C * c.N <= 1 << 16]
GEN_CLIPS = 16


def case_inputs(case):
    """x (B, C, N), idx (B, N, K) with edge 0 = the node itself, g (B, 2C, N): float32 / int64, closed-form.  Beyond 16 clips
    the values of the first 16 repeat (the hash is the slow part of a large case), x raised by 1/4 and g negated from one
    group of 16 to the next so that no two clips are equal; every clip has edges of its own."""
    B, C, N, K = case.B, case.C, case.N, case.K
    nb = min(B, GEN_CLIPS)
    assert B % nb == 0
    x = np.round(4.0 * hash_normalish(f"mr:{case.name}.x", (nb, C, N))) / 4.0
    g = np.clip(np.round(hash_normalish(f"mr:{case.name}.g", (nb, 2 * C, N)) / G_STEP) * G_STEP, -G_MAX, G_MAX)
    group = np.arange(B // nb, dtype=np.float32)[:, None, None, None]
    x = (x[None] + 0.25 * group).astype(np.float32).reshape(B, C, N)
    g = (g[None] * (1.0 - 2.0 * (group % 2.0))).astype(np.float32).reshape(B, 2 * C, N)
    idx = hash_ints(f"mr:{case.name}.idx", (B, N, K), 0, N - 1).astype(np.int64)
    idx[:, :, 0] = np.arange(N)[None, :]
    return x, idx, g


def check_grid(case, g):
    """What the exactness argument above needs of the gradients: on the 2^-4 grid, |g| <= 3, bf16 values, and every
    partial sum a node can receive below 2^15."""
    assert np.array_equal(np.round(g * 16.0), g * 16.0) and float(np.abs(g).max()) <= G_MAX
    assert np.array_equal((g.view(np.uint32) & np.uint32(0xFFFF)), np.zeros(g.shape, np.uint32))      # bf16 holds them
    assert G_MAX * case.N + 2 * G_MAX < 2 ** 15


def first_max_edge(rel):
    """The kernels' routing rule on differences (..., K), spelled out: edge 0 wins unconditionally, a later edge only on
    v > best.  np.argmax wherever no difference is NaN; a NaN wins on edge 0 only (np.argmax takes the first NaN anywhere)."""
    k, best = np.zeros(rel.shape[:-1], np.int64), rel[..., 0].copy()
    for e in range(1, rel.shape[-1]):
        wins = rel[..., e] > best
        k[wins], best[wins] = e, rel[..., e][wins]
    return k


def mr_ref(x, idx, g, block=16, winner_of=functools.partial(np.argmax, axis=-1)):
    """out (B, 2C, N) and dx (B, C, N) in float32: channel 2c = x[c], channel 2c+1 = max_k (x[c, idx] - x[c]); the
    gradient of the odd channel goes to the FIRST maximum (np.argmax) by np.add.at.  Clip block by clip block."""
    B, C, N = x.shape
    out = np.empty((B, 2 * C, N), np.float32)
    dx = np.empty((B, C, N), np.float32)
    ci = np.arange(C)[None, :, None]
    for b0 in range(0, B, block):
        xs, ii = x[b0:b0 + block], idx[b0:b0 + block]
        bi = np.arange(xs.shape[0])[:, None, None]
        rel = xs[bi[..., None], ci[..., None], ii[:, None, :, :]] - xs[..., None]              # (b, C, N, K)
        k = winner_of(rel)
        out[b0:b0 + block, 0::2] = xs
        out[b0:b0 + block, 1::2] = np.take_along_axis(rel, k[..., None], axis=-1)[..., 0]
        ge, go = g[b0:b0 + block, 0::2], g[b0:b0 + block, 1::2]
        d = ge - go
        winner = np.take_along_axis(np.broadcast_to(ii[:, None], rel.shape), k[..., None], axis=-1)[..., 0]
        np.add.at(d, (np.broadcast_to(bi, k.shape), np.broadcast_to(ci, k.shape), winner), go)
        dx[b0:b0 + block] = d
    return out, dx


@functools.lru_cache(maxsize=None)
def cached_case(name):
    """(x, idx, g), (out, dx) of a case, computed once per process and shared read-only."""
    inputs = case_inputs(CASE_BY_NAME[name])
    ref = mr_ref(*inputs)
    for a in inputs + ref:
        a.setflags(write=False)
    return inputs, ref
