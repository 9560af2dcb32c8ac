"""numpy restatement of the half form's rounding: f32 -> bf16 bit patterns, round to nearest even (what
torch.Tensor.to(torch.bfloat16) and ops.rows_to_bf16 do), and back (exact).  No torch, no GPU."""
import numpy as np


def bf16_bits(x):
    """f32 array -> uint16 array of the same shape: the bf16 nearest to each value, ties to the even mantissa; a value
    past the largest finite bf16 becomes the infinity of its sign, a NaN the quiet NaN 0x7fc0 (no fingerprint is one)."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), bits)


def bf16_values(bits):
    """uint16 bf16 bit patterns -> their f32 values (exact: a bf16 is the upper half of its f32)."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(x):
    """f32 array -> the f32 values of its bf16 rounding: U of the half form's contract."""
    return bf16_values(bf16_bits(x))
