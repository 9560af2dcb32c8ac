"""GPU tests of the NT-Xent kernels (grafp_amd/csrc/ntxent.hip) on every split plan and on ragged local ranges, against
the float64 reference of tests/_ntxent_ref.py with the bars stated there.  tests/test_ntxent_cpu.py shows through
grafp_ntxent_plan which launch regime every case of the table reaches.  Every comparison prints its worst
error-to-bar ratio (<= 1 passes).  `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

import _ntxent_ref as nr

pytestmark = pytest.mark.gpu

GUARD_BYTES, GUARD_BYTE = 4096, 0xA5           # behind the workspace
GUARD_ROWS, GUARD_VALUE = 32, 12345.0          # behind loss_partial, dzi and dzj


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.tensor(np.asarray(a), device=dev)                  # a copy: the cached inputs stay read-only


def _entry(zi, zj, B_all, D, row_begin, n_local, tau, part, dzi, dzj, ws, ws_bytes):
    from grafp_amd import ops
    p = ops._p
    return ops.lib.grafp_ntxent_fwd_bwd_f32(p(zi), p(zj), B_all, D, row_begin, n_local, float(tau), p(part), p(dzi), p(dzj),
                                            p(ws), ws_bytes, ops._stream())


def _abi(dev, zi, zj, tau, row_begin=0, n_local=None, ws_bytes=None, D=None, guard=False):
    """One call of grafp_ntxent_fwd_bwd_f32 with loss_partial, dzi and dzj pre-filled with NaN (an unwritten element
    shows) and the workspace with 0xFF bytes (NaN as f32).  Each of the three outputs is followed, in its own allocation,
    by 32 rows (loss_partial: 32 elements) of a fixed value, which must come back untouched: the gradient store of a
    ragged last block stops at n_local.  Returns (rc, loss_partial, dzi, dzj, the workspace's guard bytes or None) as numpy
    arrays.  ws_bytes: the size TOLD to the entry (default: what grafp_ntxent_workspace reports, which is also what is
    allocated in front of the workspace's own guard)."""
    from grafp_amd import ops
    lib = ops.lib
    B_all = zi.shape[0]
    D = zi.shape[1] if D is None else D
    n_local = B_all if n_local is None else n_local
    rows = max(n_local, 1)
    npart = lib.grafp_ntxent_num_partials(rows)
    nan = float("nan")
    part = torch.full((npart + GUARD_ROWS,), nan, dtype=torch.float32, device=dev)
    out = torch.full((2, rows + GUARD_ROWS, zi.shape[1]), nan, dtype=torch.float32, device=dev)
    part[npart:] = GUARD_VALUE
    out[:, rows:] = GUARD_VALUE
    nbytes = lib.grafp_ntxent_workspace(B_all)
    ws = torch.full((nbytes + GUARD_BYTES,), 0xFF, dtype=torch.uint8, device=dev)
    ws[nbytes:] = GUARD_BYTE
    assert ws.data_ptr() % 16 == 0 and out[0, :rows].is_contiguous() and out[1, :rows].is_contiguous()
    rc = _entry(_t(zi, dev), _t(zj, dev), B_all, D, row_begin, n_local, tau, part[:npart], out[0, :rows], out[1, :rows], ws,
                nbytes if ws_bytes is None else ws_bytes)
    torch.cuda.synchronize()
    assert bool((part[npart:] == GUARD_VALUE).all()), "a kernel wrote past loss_partial"
    assert bool((out[0, rows:] == GUARD_VALUE).all()), "a kernel wrote past the n_local rows of dzi"
    assert bool((out[1, rows:] == GUARD_VALUE).all()), "a kernel wrote past the n_local rows of dzj"
    return (rc, part[:npart].cpu().numpy(), out[0, :rows].cpu().numpy(), out[1, :rows].cpu().numpy(),
            ws[nbytes:].cpu().numpy() if guard else None)


def _ops_call(dev, zi, zj, tau, row_begin=None, n_local=None, scale=None):
    """ops.ntxent + backward; the local form when row_begin is given.  Returns (loss, dzi, dzj) as numpy (loss f32)."""
    from grafp_amd import ops
    if row_begin is None:
        a, b = _t(zi, dev).requires_grad_(True), _t(zj, dev).requires_grad_(True)
        loss = ops.ntxent(a, b, tau)
    else:
        zi_all, zj_all = _t(zi, dev), _t(zj, dev)
        a = zi_all[row_begin:row_begin + n_local].clone().requires_grad_(True)
        b = zj_all[row_begin:row_begin + n_local].clone().requires_grad_(True)
        loss = ops.ntxent(a, b, tau, zi_all, zj_all, row_begin)
    (loss if scale is None else scale * loss).backward()
    return loss.detach().cpu().numpy(), a.grad.cpu().numpy(), b.grad.cpu().numpy()


_GLOBAL = {}


def _kernel_global(dev, B, D, tau, kind):
    """The kernels' own full-form result of a case's inputs, computed once and shared."""
    key = (B, D, tau, kind)
    if key not in _GLOBAL:
        zi, zj = nr.inputs(B, D, kind)
        _GLOBAL[key] = _ops_call(dev, zi, zj, tau)
    return _GLOBAL[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _against_f64(c, ref, sc, row_begin, n_local, loss, part, dzi, dzj, what):
    """The ratios of every checked quantity to its bar; prints the worst and asserts all of them <= 1."""
    loc = nr.local_f64(ref, row_begin, n_local)
    M = 2 * c.B
    pbars = nr.partial_bars(ref, sc, row_begin, n_local)
    ratios = {
        "partials": nr.worst(part, loc.partials, pbars),
        "loss": nr.worst(loss, loc.share, pbars.sum() / M),
        "partials' sum": nr.worst(part.astype(np.float64).sum() / M, loc.share, pbars.sum() / M),
        "dzi": nr.worst(dzi, loc.dzi, nr.grad_bar(loc.dzi, sc)),
        "dzj": nr.worst(dzj, loc.dzj, nr.grad_bar(loc.dzj, sc)),
    }
    print(f"ntxent {what} {nr.case_id(c)}: worst error / bar " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items())
          + f"  -> {max(ratios.values()):.3f}")
    assert max(ratios.values()) <= 1.0, ratios
    return ratios


# ================================================================================================ full form
@pytest.mark.parametrize("c", nr.FULL_CASES, ids=nr.case_id)
def test_full_form_vs_float64(dev, c):
    """Loss partials, loss, dzi and dzj of every full-form case, through ops.ntxent and through the C entry (outputs
    pre-filled with NaN), against float64.  Bars (tests/_ntxent_ref.py): per row 2e-5 |lse - pos| + 8 * 2^-23 * Lmax, a partial
    the sum of its rows' bars, the loss the same divided by 2B; gradients 1e-4 |want| + 1e-5 G0."""
    from grafp_amd import ops
    zi, zj = nr.inputs(c.B, c.D, c.kind)
    ref, sc = nr.cached_ref(c.B, c.D, c.tau, c.kind), nr.scales(zi, zj, c.tau)
    loss, gi, gj = _kernel_global(dev, c.B, c.D, c.tau, c.kind)
    rc, part, dzi, dzj, _ = _abi(dev, zi, zj, c.tau)
    assert rc == 0, ops.lib.grafp_last_error()
    assert len(part) == nr.plan(ops.lib, c.B, c.B).partials
    # the autograd surface hands out the C entry's gradients unchanged (unit upstream gradient)
    assert np.array_equal(_bits(gi), _bits(dzi)) and np.array_equal(_bits(gj), _bits(dzj))
    _against_f64(c, ref, sc, 0, c.B, loss, part, dzi, dzj, "full")
    if c.B == 1:                                                    # the only candidate is the partner
        assert ref.loss == 0.0 and float(loss) == 0.0 and not part[:2].any() and not dzi.any() and not dzj.any()
    else:
        assert ref.loss > 1e-6                                       # a loss that can be wrong


# ================================================================================================ local form
@pytest.mark.parametrize("c", nr.LOCAL_CASES, ids=nr.case_id)
def test_local_form_vs_float64_and_the_global_gradient(dev, c):
    """Ragged local ranges (n_local % 32 != 0, 32-row blocks off the 32-row grid, a range that ends at B_all, one row):
    against the float64 local reference, and against the matching slice of the kernels' own global gradient at the
    rtol 1e-5 of test_ntxent_local_rows_global_columns (the summation order differs where pass 2's split count does)."""
    from grafp_amd import ops
    zi, zj = nr.inputs(c.B, c.D, c.kind)
    ref, sc = nr.cached_ref(c.B, c.D, c.tau, c.kind), nr.scales(zi, zj, c.tau)
    lo, hi = c.row_begin, c.row_begin + c.n_local
    loss, gi, gj = _ops_call(dev, zi, zj, c.tau, c.row_begin, c.n_local)
    rc, part, dzi, dzj, _ = _abi(dev, zi, zj, c.tau, c.row_begin, c.n_local)
    assert rc == 0, ops.lib.grafp_last_error()
    assert gi.shape == (c.n_local, c.D) and len(part) == nr.plan(ops.lib, c.B, c.n_local).partials
    assert np.array_equal(_bits(gi), _bits(dzi)) and np.array_equal(_bits(gj), _bits(dzj))
    _against_f64(c, ref, sc, c.row_begin, c.n_local, loss, part, dzi, dzj, "local")
    _, full_i, full_j = _kernel_global(dev, c.B, c.D, c.tau, c.kind)
    np.testing.assert_allclose(dzi, full_i[lo:hi], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(dzj, full_j[lo:hi], rtol=1e-5, atol=1e-8)


def test_local_losses_of_a_ragged_partition_sum_to_the_global_loss(dev):
    B, D, tau = 520, 128, 0.05
    zi, zj = nr.inputs(B, D, "unit")
    ref, sc = nr.cached_ref(B, D, tau, "unit"), nr.scales(zi, zj, tau)
    full, _, _ = _kernel_global(dev, B, D, tau, "unit")
    total = sum(float(_ops_call(dev, zi, zj, tau, lo, n)[0]) for lo, n in nr.PARTITION_520)
    ratio = nr.worst(total, ref.loss, nr.loss_bar(ref.loss, sc))     # the parts' bars add up to the loss bar
    print(f"ntxent partition of 520: sum of the local losses {total:.9g}, global {float(full):.9g}, float64 {ref.loss:.12g}; "
          f"error / bar {ratio:.3f}")
    assert ratio <= 1.0
    np.testing.assert_allclose(total, float(full), rtol=1e-5)


# ================================================================================================ workspace
@pytest.mark.parametrize("B,D,row_begin,n_local", [(520, 128, 0, 520), (1100, 128, 0, 1100), (1100, 128, 963, 137)])
def test_kernels_stay_inside_the_reported_workspace(dev, B, D, row_begin, n_local):
    """A workspace of exactly grafp_ntxent_workspace(B_all) bytes followed, in the same allocation, by a 4 KB guard of a
    fixed byte: the guard is untouched, the results are those of float64.  One byte less is refused before any launch."""
    from grafp_amd import ops
    zi, zj = nr.inputs(B, D, "unit")
    ref, sc = nr.cached_ref(B, D, 0.05, "unit"), nr.scales(zi, zj, 0.05)
    rc, part, dzi, dzj, guard = _abi(dev, zi, zj, 0.05, row_begin, n_local, guard=True)
    assert rc == 0, ops.lib.grafp_last_error()
    assert guard.shape == (GUARD_BYTES,) and bool((guard == GUARD_BYTE).all()), "a kernel wrote past the workspace"
    c = nr.Local(B, D, 0.05, "unit", row_begin, n_local)
    _against_f64(c, ref, sc, row_begin, n_local, part.astype(np.float64).sum() / (2 * B), part, dzi, dzj, "guarded")
    nbytes = ops.lib.grafp_ntxent_workspace(B)
    rc, part, dzi, dzj, guard = _abi(dev, zi, zj, 0.05, row_begin, n_local, ws_bytes=nbytes - 1, guard=True)
    assert rc == -2 and b"workspace" in ops.lib.grafp_last_error()                       # GRAFP_ERR_WORKSPACE
    assert np.isnan(part).all() and np.isnan(dzi).all() and np.isnan(dzj).all() and bool((guard == GUARD_BYTE).all())


# ================================================================================================ determinism
@pytest.mark.parametrize("B,D,row_begin,n_local", [(520, 128, 0, 520), (1100, 64, 963, 137)])
def test_two_calls_give_equal_bits(dev, B, D, row_begin, n_local):
    zi, zj = nr.inputs(B, D, "unit")
    first = _abi(dev, zi, zj, 0.05, row_begin, n_local)
    second = _abi(dev, zi, zj, 0.05, row_begin, n_local)
    assert first[0] == 0 and second[0] == 0
    for a, b in zip(first[1:4], second[1:4]):
        assert not np.isnan(a).any() and np.array_equal(_bits(a), _bits(b))


# ================================================================================================ autograd surface
def test_upstream_gradient_scales_the_gradients_exactly(dev):
    zi, zj = nr.inputs(193, 128, "unit")
    loss1, gi1, gj1 = _ops_call(dev, zi, zj, 0.05)
    loss2, gi2, gj2 = _ops_call(dev, zi, zj, 0.05, scale=2.5)
    assert np.array_equal(_bits(loss1), _bits(loss2))
    assert np.array_equal(_bits(gi2), _bits(np.float32(2.5) * gi1)) and np.array_equal(_bits(gj2), _bits(np.float32(2.5) * gj1))
    assert np.abs(gi1).max() > 0


def test_bf16_inputs_under_autocast_equal_their_f32_widening(dev):
    from grafp_amd import ops
    zi, zj = nr.inputs(70, 64, "unit")
    a16 = _t(zi, dev).to(torch.bfloat16).requires_grad_(True)
    b16 = _t(zj, dev).to(torch.bfloat16).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss16 = ops.ntxent(a16, b16, 0.05)
    loss16.backward()
    a32 = a16.detach().float().requires_grad_(True)
    b32 = b16.detach().float().requires_grad_(True)
    loss32 = ops.ntxent(a32, b32, 0.05)
    loss32.backward()
    assert loss16.dtype == torch.float32 and torch.equal(loss16.detach(), loss32.detach())
    # autograd hands a bf16 leaf its gradient in bf16: the f32 gradient, rounded once
    assert a32.grad.abs().max() > 0
    assert torch.equal(a16.grad.float(), a32.grad.to(a16.grad.dtype).float())
    assert torch.equal(b16.grad.float(), b32.grad.to(b16.grad.dtype).float())


# ================================================================================================ NaN
def test_one_nan_input_poisons_what_the_reference_says_it_poisons(dev):
    """One NaN in one row of zi (no inf, nothing else poisoned): the loss is NaN and the gradients are NaN wherever the
    float64 reference's are -- the positions are the reference's, not assumed."""
    B, D, tau = 193, 128, 0.05
    zi, zj = nr.inputs(B, D, "unit")
    zi = zi.copy()
    zi[57, 5] = np.nan
    ref = nr.ntxent_f64(zi, zj, tau)
    sc = nr.scales(zi, zj, tau)
    assert np.isnan(ref.loss) and np.isnan(ref.dzi).any()
    loss, gi, gj = _ops_call(dev, zi, zj, tau)
    rc, part, dzi, dzj, _ = _abi(dev, zi, zj, tau)
    assert rc == 0 and np.isnan(loss)
    loc = nr.local_f64(ref, 0, B)
    assert np.array_equal(np.isnan(part), np.isnan(loc.partials))
    for got, want in ((gi, ref.dzi), (gj, ref.dzj), (dzi, ref.dzi), (dzj, ref.dzj)):
        bad = np.isnan(want)
        assert np.array_equal(np.isnan(got), bad), (int(np.isnan(got).sum()), int(bad.sum()))
        if (~bad).any():                                             # what the reference keeps finite is still right
            assert nr.worst(got[~bad], want[~bad], nr.grad_bar(want, sc)[~bad]) <= 1.0


# ================================================================================================ refusals
@pytest.mark.parametrize("D,tau,row_begin,n_local", [(16, 0.05, 0, 8), (160, 0.05, 0, 8), (48, 0.05, 0, 8), (128, 0.0, 0, 8),
                                                     (128, -0.05, 0, 8), (128, 0.05, 5, 4), (128, 0.05, 0, 0)])
def test_refused_arguments_raise_and_launch_nothing(dev, D, tau, row_begin, n_local):
    from grafp_amd import ops
    B = 8
    zi = np.ascontiguousarray(nr.inputs(B, 128, "unit")[0][:, :1].repeat(D, axis=1))
    zj = zi.copy()
    rc, part, dzi, dzj, guard = _abi(dev, zi, zj, tau, row_begin, n_local, guard=True)
    assert rc == -1, rc                                                                  # GRAFP_ERR_ARG
    assert np.isnan(part).all() and np.isnan(dzi).all() and np.isnan(dzj).all() and bool((guard == GUARD_BYTE).all())
    zi_all, zj_all = _t(zi, dev), _t(zj, dev)
    local = torch.zeros(n_local, D, device=dev)
    with pytest.raises(RuntimeError, match="ntxent"):
        ops.ntxent(local, local.clone(), tau, zi_all, zj_all, row_begin)
    if row_begin == 0 and n_local == B:
        with pytest.raises(RuntimeError, match="ntxent"):
            ops.ntxent(zi_all, zj_all, tau)


# ================================================================================================ the wrapper's checks
def test_wrapper_refuses_mismatched_shapes_before_any_launch(dev):
    """ops.ntxent reads zi_all and zj_all with z_i's width and zi_all's row count: every mismatch is a ValueError that names
    the shapes (device tensors, no kernel launched)."""
    from grafp_amd import ops
    z = lambda *s: torch.zeros(*s, device=dev)                       # noqa: E731
    calls = {
        "z_i / z_j shapes": (lambda: ops.ntxent(z(8, 128), z(8, 64), 0.05), r"\(8, 128\).*\(8, 64\)"),
        "z_i / z_j rows": (lambda: ops.ntxent(z(8, 128), z(7, 128), 0.05), r"\(8, 128\).*\(7, 128\)"),
        "not 2-D": (lambda: ops.ntxent(z(2, 4, 128), z(2, 4, 128), 0.05), r"\(2, 4, 128\)"),
        "only zi_all": (lambda: ops.ntxent(z(4, 128), z(4, 128), 0.05, z(8, 128), None, 0), r"only zi_all.*\(8, 128\)"),
        "only zj_all": (lambda: ops.ntxent(z(4, 128), z(4, 128), 0.05, None, z(8, 128), 0), r"only zj_all.*\(8, 128\)"),
        "zi_all / zj_all shapes": (lambda: ops.ntxent(z(4, 128), z(4, 128), 0.05, z(8, 128), z(6, 128), 0),
                                   r"\(8, 128\).*\(6, 128\)"),
        "zj_all narrower": (lambda: ops.ntxent(z(4, 128), z(4, 128), 0.05, z(8, 128), z(8, 64), 0), r"\(8, 128\).*\(8, 64\)"),
        "width of the gathered": (lambda: ops.ntxent(z(4, 128), z(4, 128), 0.05, z(8, 64), z(8, 64), 0),
                                  r"\(8, 64\).*\(4, 128\)"),
        "gathered not 2-D": (lambda: ops.ntxent(z(4, 128), z(4, 128), 0.05, z(8, 1, 128), z(8, 1, 128), 0), r"\(8, 1, 128\)"),
        "another device": (lambda: ops.ntxent(z(4, 128), z(4, 128), 0.05, torch.zeros(8, 128), torch.zeros(8, 128), 0),
                           r"cpu"),
    }
    for call, pattern in calls.values():
        with pytest.raises(ValueError, match=pattern):
            call()
