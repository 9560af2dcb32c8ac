"""Edge values of the f32 -> bf16 stores of csrc/elemio.h, bit for bit against torch's CPU conversion.  `pytest -m gpu`.

Two conversions exist: the scalar integer form f32_to_bf16 and the hardware pair form pack_bf16.
Both round to nearest even and keep a NaN a NaN; every path below stores through one of them.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ZEROS = [0x00000000, 0x80000000]
TIES = [0x3f808000,     # tie, rounds to even: down
        0x3f818000,     # tie, rounds up
        0x3f807fff, 0x3f808001]     # either side of a tie
LARGE = [0x7f7f0000,    # largest bf16, unchanged
         0x7f7fffff]    # rounds to +inf
INFS = [0x7f800000, 0xff800000]
NANS = [0x7fc00000, 0x7f800001, 0xffffffff]     # the second: payload only in the low bits
DENORMALS = [0x00000001, 0x00008000, 0x00018000, 0x00010000]
ALL = ZEROS + TIES + LARGE + INFS + NANS + DENORMALS
# bf16-representable normals, inf and NaN: what a load -> unpack -> pack -> store round trip must hand back unchanged
ROUND_TRIP = [0x3f800000, 0x3f810000, 0xbf800000, 0x7f7f0000, 0xff7f0000, 0x00800000, 0x40490000] + INFS + [0x7fc00000]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _f32(bits, n=None):
    """f32 tensor of the bit patterns, padded to n elements by repetition"""
    a = np.asarray(bits, dtype=np.uint32)
    if n is not None:
        a = np.resize(a, n)
    return torch.from_numpy(a.view(np.float32).copy())


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16)


def _is_nan16(b):
    return ((b & 0x7f80) == 0x7f80) & ((b & 0x007f) != 0)


def _assert_bf16_bits(got_bf16, want_bf16, what):
    """stored bit patterns equal; NaN compares as "is NaN\""""
    got, want = _bits16(got_bf16).ravel(), _bits16(want_bf16).ravel()
    gn, wn = _is_nan16(got), _is_nan16(want)
    bad = (gn != wn) | (~wn & (got != want))
    assert not bad.any(), f"{what}: " + ", ".join(f"[{i}] got {got[i]:#06x} want {want[i]:#06x}" for i in np.flatnonzero(bad)[:8])


def _bf16_pair_with_sum(p):
    """two bf16 values (as f32 tensors of one element) whose f32 sum has the bit pattern p, or None"""
    hi = p & 0xffff0000
    for a_bits in (hi, (hi + 0x10000) & 0xffffffff, (hi - 0x10000) & 0xffffffff):
        a = _f32([a_bits])
        b = _f32([p]) - a
        if not torch.isfinite(a).all() or not torch.isfinite(b).all():
            continue
        if (b.view(torch.int32) & 0xffff).item() == 0 and (a + b).view(torch.int32).item() == _f32([p]).view(torch.int32).item():
            return a, b
    return None


def _taps_case(N, patterns):
    """The gradient (3, 2, 1, n_out) of ops.stride2_taps for an input (2, 1, N) in which every pattern that can be made
    arrives at one input position: a bf16-representable one through an EVEN position (tap 1 alone), any other as the f32
    sum tap2 + tap0 at an ODD position.  Returns (g f32 holding bf16 values, expected dx f32 before rounding, the patterns
    placed, the patterns that cannot be made)."""
    n_out = (N - 1) // 2 + 1
    g = torch.zeros((3, 2, 1, n_out), dtype=torch.float32)
    want = torch.zeros((2, 1, N), dtype=torch.float32)
    even = [(r, j) for r in range(2) for j in range(n_out)]
    odd = [(r, j) for r in range(2) for j in range(n_out - 1) if 2 * j + 1 < N]
    placed, impossible = [], []
    for p in patterns:
        if p & 0xffff == 0:
            r, j = even.pop(0)
            g[1, r, 0, j] = _f32([p])[0]
            want[r, 0, 2 * j] = _f32([p])[0]
            placed.append(p)
            continue
        pair = _bf16_pair_with_sum(p)
        if pair is None:
            impossible.append(p)
            continue
        r, j = odd.pop(0)
        g[2, r, 0, j], g[0, r, 0, j + 1] = pair[0][0], pair[1][0]
        want[r, 0, 2 * j + 1] = pair[0][0] + pair[1][0]
        placed.append(p)
    return g, want, placed, impossible


# The f32 sum of two bf16 values cannot have these patterns (each summand has 8 significant bits, and both must lie within
# a few bf16 steps of the sum's top half for the low half to survive; a NaN that comes out of an f32 addition is either
# an input's, with its payload in the bf16 half, or the default 0x7fc00000): they reach the scalar conversion through
# ops.rows_to_bf16 below, never through a bf16 gradient.
TAPS_UNREACHABLE = [0x3f807fff, 0x3f808001, 0x7f7fffff, 0x7f800001, 0xffffffff, 0x00000001, 0x00008000, 0x00018000]


def _taps_bwd(dev, g, N):
    from grafp_amd import ops
    x = torch.zeros((2, 1, N), dtype=torch.bfloat16, device=dev, requires_grad=True)
    out = ops.stride2_taps(x)
    assert tuple(out.shape) == tuple(g.shape)
    out.backward(g.to(torch.bfloat16).to(dev))
    return x.grad


def test_bf16_store_edge_values(dev):
    """Every bf16 store path against torch's CPU x.to(torch.bfloat16), bit patterns compared."""
    from grafp_amd import ops

    # --- the scalar integer form: ops.rows_to_bf16, all patterns (denormals and NaNs included), one row of 128
    x = _f32(ALL, 128).reshape(1, 128)
    _assert_bf16_bits(ops.rows_to_bf16(x.to(dev)), x.to(torch.bfloat16), "rows_to_bf16")

    # --- ops.stride2_taps bf16 backward: (2, 1, 16) runs the 8-wide kernels (pair form), (2, 1, 10) the scalar ones
    for N, patterns in ((16, [p for p in ALL if p not in DENORMALS]), (10, ALL)):
        g, want, placed, impossible = _taps_case(N, patterns)
        assert sorted(impossible) == sorted(p for p in TAPS_UNREACHABLE if p in patterns), [hex(p) for p in impossible]
        _assert_bf16_bits(g.to(torch.bfloat16), (g.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16), "g is bf16 as built")
        assert (g.view(torch.int32) & 0xffff == 0).all()
        dx = _taps_bwd(dev, g, N)
        assert dx.dtype == torch.bfloat16 and tuple(dx.shape) == (2, 1, N)
        _assert_bf16_bits(dx, want.to(torch.bfloat16), f"stride2_taps backward N={N} ({[hex(p) for p in placed]})")
    # what the pair form does with a bf16 denormal (not asserted: BatchNorm and max-relative depend on it as it is)
    g, want, _, _ = _taps_case(16, [0x00010000])
    print("pair form, bf16 denormal 0x0001 through stride2_taps backward (2, 1, 16): "
          f"{_bits16(_taps_bwd(dev, g, 16)).ravel()[0]:#06x}")

    # --- ops.split_planes, the hi plane (pair form straight from f32): finite patterns, inf and NaNs
    pats = ZEROS + TIES + LARGE + INFS + NANS
    x = _f32(pats, 16)
    hi, _ = ops.split_planes(x.to(dev))
    _assert_bf16_bits(hi, x.to(torch.bfloat16), "split_planes hi")
    hi, _ = ops.split_planes(_f32(DENORMALS, 8).to(dev))
    print("pair form, f32 denormals", [hex(p) for p in DENORMALS], "through split_planes hi:",
          [f"{b:#06x}" for b in _bits16(hi).ravel()[:4]], "torch:",
          [f"{b:#06x}" for b in _bits16(_f32(DENORMALS).to(torch.bfloat16))])

    # --- round trips of bf16-representable values: the stored bits are the bits given
    # BatchNorm in eval mode with mean 0, variance 1 - eps, gamma 1, beta 0 and no activation (the 16-byte piece) ...
    eps = 1e-5
    xb = _f32(ROUND_TRIP, 32).reshape(2, 16).to(torch.bfloat16)
    ones, zeros = torch.ones(2, device=dev), torch.zeros(2, device=dev)
    z = ops.bn_act(xb.to(dev), ones, zeros, zeros.clone(), torch.full((2,), 1.0 - eps, device=dev), False, eps=eps,
                   act=ops.ACT_NONE)
    _assert_bf16_bits(z, xb, "bn_act eval identity")
    # ... and max-relative with K = 1, whose even output channels are a copy of x (the 4-element piece)
    xm = _f32(ROUND_TRIP, 32).reshape(1, 4, 8).to(torch.bfloat16)
    idx = torch.arange(8, dtype=torch.int64).reshape(1, 8, 1)
    out = ops.max_relative(xm.to(dev), idx.to(dev))
    assert tuple(out.shape) == (1, 8, 8)
    _assert_bf16_bits(out[:, 0::2], xm, "max_relative even channels")


@pytest.mark.parametrize("N", [16, 10])
def test_stride2_taps_nan_gradient_stays_nan(dev, N):
    """A NaN in the f32 sum of the stride2_taps bf16 backward comes out a NaN at exactly the input position its taps feed.
    Row 0: tap 2 of output 1 is a NaN (feeds position 3).  Row 1: tap 2 of output 2 is +inf and tap 0 of output 3 is -inf:
    the NaN exists only as their sum (position 5).  (A NaN with its payload only in the LOW bits, 0x7f800001, cannot reach
    this conversion from bf16 inputs -- see TAPS_UNREACHABLE; the parent's unguarded conversion turned that one into inf,
    which test_bf16_store_edge_values checks through ops.rows_to_bf16.)"""
    n_out = (N - 1) // 2 + 1
    g = ((torch.arange(3 * 2 * n_out, dtype=torch.float32) % 7) - 3.0).reshape(3, 2, 1, n_out)
    g[2, 0, 0, 1] = float("nan")
    g[2, 1, 0, 2], g[0, 1, 0, 3] = float("inf"), float("-inf")
    dx = _taps_bwd(dev, g, N).float().cpu()
    want = torch.zeros((2, 1, N), dtype=torch.bool)
    want[0, 0, 3] = True
    want[1, 0, 5] = True
    assert torch.equal(torch.isnan(dx), want), torch.isnan(dx).nonzero().tolist()
    assert torch.isfinite(dx[~want]).all()
