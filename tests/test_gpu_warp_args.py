"""The argument handling ops.speed_change and ops.time_stretch share (ops._warp_args), on the device: what it refuses, by
message, and the forms of x and ratio it takes, each held bit for bit against the plain (B, T_in) f32 call.  The shapes
are the smallest that reach every branch: 3 clips of 700 samples, 300 outputs -- one tile of the speed kernel, three
frames of the stretch."""
import pytest
import torch

from grafp_amd import ops

pytestmark = pytest.mark.gpu
B, T_IN, OUT_LEN, OFF = 3, 700, 300, 20
OPS = {"speed_change": ops.speed_change, "time_stretch": ops.time_stretch}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case(dev):
    """x, the per-clip ratios (below 1, exactly 1: the copy branch, above 1) and each op's plain result"""
    x = (0.5 * torch.randn(B, T_IN, generator=torch.Generator().manual_seed(17))).to(dev)
    ratio = torch.tensor([0.97, 1.0, 1.05], device=dev)
    return x, ratio, {name: op(x, ratio, OUT_LEN, OFF) for name, op in OPS.items()}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", OPS)
def test_refusals_name_the_op(dev, case, name):
    op, (x, ratio, _) = OPS[name], case
    with pytest.raises(ValueError, match=rf"^{name}: x must be \(B, T_in\) or \(T_in,\)$"):
        op(x.reshape(B, 1, T_IN), ratio, OUT_LEN, OFF)
    with pytest.raises(ValueError, match=rf"^{name}: 2 ratios for 3 clips$"):
        op(x, ratio[:2], OUT_LEN, OFF)
    bad_out = rf"^{name}: `out` must be a \(B, out_len\) f32 device tensor with unit column stride$"
    for out in (torch.empty(B, OUT_LEN - 1, device=dev),                              # the wrong shape
                torch.empty(B, OUT_LEN, device=dev, dtype=torch.float64),             # the wrong dtype
                torch.empty(B, 2 * OUT_LEN, device=dev)[:, ::2],                      # a column stride of 2
                torch.empty(1, OUT_LEN, device=dev).expand(B, OUT_LEN)):              # a row stride of 0 < out_len
        with pytest.raises(ValueError, match=bad_out):
            op(x, ratio, OUT_LEN, OFF, out=out)


@pytest.mark.parametrize("name", OPS)
def test_a_1d_x_is_row_zero_and_comes_back_1d(dev, case, name):
    op, (x, ratio, want) = OPS[name], case
    y = op(x[0], ratio[:1], OUT_LEN, OFF)
    assert y.shape == (OUT_LEN,) and _same_bits(y, want[name][0])
    out = torch.full((1, OUT_LEN), float("nan"), device=dev)
    y = op(x[0], ratio[:1], OUT_LEN, OFF, out=out)
    assert y.shape == (OUT_LEN,) and y.data_ptr() == out.data_ptr() and _same_bits(y, want[name][0])


@pytest.mark.parametrize("name", OPS)
def test_out_is_written_in_place_and_returned(dev, case, name):
    op, (x, ratio, want) = OPS[name], case
    wide = torch.full((B, OUT_LEN + 5), float("nan"), device=dev)
    y = op(x, ratio, OUT_LEN, OFF, out=wide[:, :OUT_LEN])
    assert y.data_ptr() == wide.data_ptr() and _same_bits(y, want[name])
    assert bool(torch.isnan(wide[:, OUT_LEN:]).all())


@pytest.mark.parametrize("name", OPS)
def test_a_scalar_ratio_is_a_tensor_full_of_it(dev, case, name):
    op, (x, _, _) = OPS[name], case
    assert _same_bits(op(x, 1.05, OUT_LEN, OFF), op(x, torch.full((B,), 1.05, device=dev), OUT_LEN, OFF))


@pytest.mark.parametrize("name", OPS)
def test_a_float64_x_is_its_f32_copy(dev, case, name):
    op, (x, ratio, _) = OPS[name], case
    x64 = x.double() + 1e-12                                 # not representable in f32: the conversion rounds
    assert _same_bits(op(x64, ratio, OUT_LEN, OFF), op(x64.float(), ratio, OUT_LEN, OFF))


@pytest.mark.parametrize("name", OPS)
def test_an_expanded_row_is_its_contiguous_copy(dev, case, name):
    op, (x, ratio, want) = OPS[name], case
    rows = x[0].expand(B, T_IN)                              # row stride 0, below the row length
    assert rows.stride() == (0, 1)
    got = op(rows, ratio, OUT_LEN, OFF)
    assert _same_bits(got, op(rows.contiguous(), ratio, OUT_LEN, OFF))
    assert _same_bits(got[0], want[name][0])                 # clip 0 at ratio 0.97, as in the plain call
