"""CPU tests of what the max-relative GPU tests stand on (tests/_mrconv_ref.py): the numpy reference against the oracle,
the gradient grid that makes the comparison exact, and the launch choice of mrconv.hip through grafp_mrconv_plan (a pure
host function: no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import _mrconv_ref as mr


def _plan(dtype, x_s, o_s, B, C, N, K, aligned, backward, with_arg):
    """(rc, info[:5], LDS bytes) of grafp_mrconv_plan."""
    from grafp_amd._lib import lib
    info = (ctypes.c_int * 8)()
    rc = lib.grafp_mrconv_plan(dtype, x_s[0], x_s[1], o_s[0], o_s[1], B, C, N, K, int(aligned), int(backward), int(with_arg), info)
    assert list(info[6:8]) == [0, 0]
    return rc, tuple(info[:5]), info[5]


def _strides(case, layout):
    """(x strides, out / grad_out strides) of a case in (B, C, N) or (C, B, N) layout."""
    B, C, N = case.B, case.C, case.N
    return ((C * N, N), (2 * C * N, N)) if layout == "bcn" else ((N, B * N), (N, B * N))


@pytest.mark.parametrize("name", mr.SMALL_CASES)
def test_reference_equals_the_oracle(name):
    """Forward: equal to oracle.model.max_relative.  Backward: torch's CPU autograd of the oracle routes to the first
    maximum too, and on the gradient grid its sums are exact in any order, so dx is equal as well."""
    from oracle import model as om
    (x, idx, g), (out, dx) = mr.cached_case(name)
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    want = om.max_relative(xt, torch.from_numpy(idx.copy()))
    assert np.array_equal(want.detach().numpy(), out)
    want.backward(torch.from_numpy(g.copy()))
    assert np.array_equal(xt.grad.numpy(), dx)


@pytest.mark.parametrize("name", [c.name for c in mr.CASES])
def test_gradients_are_on_the_grid_that_makes_the_sums_exact(name):
    case = mr.CASE_BY_NAME[name]
    x, idx, g = mr.case_inputs(case)
    mr.check_grid(case, g)
    assert np.array_equal(np.round(4.0 * x), 4.0 * x) and float(np.abs(x).max()) < 8.0
    assert np.array_equal(idx[:, :, 0], np.broadcast_to(np.arange(case.N), (case.B, case.N)))
    if name in mr.SMALL_CASES:
        # the bound of check_grid (3 N) is not needed in full: the largest sum of |addends| any node receives
        _, dx = mr.cached_case(name)[1]
        assert float(np.abs(dx).max()) < 2 ** 15
        rel = x[np.arange(case.B)[:, None, None, None], np.arange(case.C)[None, :, None, None], idx[:, None]] - x[..., None]
        assert np.array_equal(mr.first_max_edge(rel), np.argmax(rel, axis=-1))          # the kernels' rule, without NaN
        ties = (rel == rel.max(axis=-1, keepdims=True)).sum(axis=-1) > 1
        assert ties.mean() > 0.02, "the coarse x grid is there for ties among the neighbours"


@pytest.mark.parametrize("name", [c.name for c in mr.CASES])
def test_plan_query_reports_the_hand_derived_launches(name):
    """Every case of the table, both dtypes and both layouts: the plan is the table's (the layouts differ in strides only,
    all multiples of 4 when N is), with and without the record; a misaligned pointer takes the 4-wide cases to scalar."""
    case = mr.CASE_BY_NAME[name]
    for dtype in (0, 1):
        for layout in ("bcn", "cbn"):
            xs, os_ = _strides(case, layout)
            aligned = not case.off1
            for backward, want in ((0, case.fwd), (1, case.bwd)):
                rc, got, lds = _plan(dtype, xs, os_, case.B, case.C, case.N, case.K, aligned, backward, 0)
                assert rc == 0 and got == want, (name, dtype, layout, backward, got)
                assert 0 < lds <= 160 * 1024
                rc, got, _ = _plan(dtype, xs, os_, case.B, case.C, case.N, case.K, aligned, backward, 1)
                assert rc == 0 and got == (case.rec[backward] if case.rec else want), (name, "record", backward, got)
                if want[0] in (mr.PERSISTENT, mr.VEC4) or case.off1:
                    rc, got, _ = _plan(dtype, xs, os_, case.B, case.C, case.N, case.K, False, backward, 1)
                    if backward and case.N > 2048:                    # more nodes than a scalar workgroup covers
                        assert rc == -1, (name, "misaligned", got)
                    else:
                        assert rc == 0 and got[0] == mr.SCALAR, (name, "misaligned", backward, got)


def test_lds_bytes_of_each_kernel():
    """rows | edges forward; i64 accumulator + rows | edges in the persistent backward; i64 accumulator | edges from the
    record, which is what the forward with the record needs too (16384 + 4 K N): grafp_mrconv_arg_supported may look at one."""
    c = mr.CASE_BY_NAME["persistent-short-last"]
    xs, os_ = _strides(c, "bcn")
    kn = 4 * c.K * c.N
    assert _plan(0, xs, os_, c.B, c.C, c.N, c.K, True, 0, 0)[2] == 16384 + kn
    assert _plan(0, xs, os_, c.B, c.C, c.N, c.K, True, 0, 1)[2] == 16384 + kn
    assert _plan(0, xs, os_, c.B, c.C, c.N, c.K, True, 1, 0)[2] == 24576 + kn
    assert _plan(0, xs, os_, c.B, c.C, c.N, c.K, True, 1, 1)[2] == 16384 + kn
    c = mr.CASE_BY_NAME["vec4-items2"]
    xs, os_ = _strides(c, "bcn")
    assert _plan(0, xs, os_, c.B, c.C, c.N, c.K, True, 1, 0)[2] == 16 * c.N + 4 * c.K * c.N == 159744
    c = mr.CASE_BY_NAME["scalar-items8"]
    xs, os_ = _strides(c, "bcn")
    assert _plan(0, xs, os_, c.B, c.C, c.N, c.K, True, 0, 0)[2] == 4 * (4 * c.N + c.K * c.N)
    assert _plan(0, xs, os_, c.B, c.C, c.N, c.K, True, 1, 0)[2] == 4 * (4 * 2 * c.N + c.K * c.N)


def test_arg_supported_is_the_plans_record_answer():
    """grafp_mrconv_arg_supported (pointer alignment aside) = the plan of an aligned call that wants the record says
    path 3, forward and backward, over a grid of N, K and strides."""
    from grafp_amd._lib import lib
    seen = set()
    for dtype in (0, 1, 7):
        for N in (0, 4, 64, 100, 101, 2048, 2052, 4096):
            for K in (0, 1, 4, 5):
                for xs in ((8 * N, N), (N, 3 * N), (8 * N + 2, N), (8 * N, N + 1)):
                    for os_ in ((16 * N, N), (16 * N, N + 2)):
                        sup = lib.grafp_mrconv_arg_supported(dtype, xs[0], xs[1], os_[0], os_[1], N, K)
                        plans = [_plan(dtype, xs, os_, 3, 8, N, K, True, backward, 1) for backward in (0, 1)]
                        rec = [rc == 0 and info[0] == mr.RECORD for rc, info, _ in plans]
                        assert rec[0] == rec[1] == bool(sup), (dtype, N, K, xs, os_, sup, plans)
                        seen.add(bool(sup))
    assert seen == {False, True}
    assert lib.grafp_mrconv_arg_supported(0, 8 * 64, 64, 16 * 64, 64, 64, 3) == 1
    assert lib.grafp_mrconv_arg_supported(0, 8 * 2052, 2052, 16 * 2052, 2052, 2052, 3) == 0


def test_plan_query_refuses_what_no_kernel_takes():
    from grafp_amd._lib import lib
    err = lambda: lib.grafp_last_error()                                                  # noqa: E731
    info = (ctypes.c_int * 8)()
    # N = 2049, scalar: a workgroup of the generic backward covers 8 x 256 nodes; the forward takes it
    assert _plan(0, (2049, 2049), (4098, 2049), 1, 1, 2049, 2, True, 1, 0)[0] == -1
    assert b"mrconv_bwd: N=2049 exceeds the 2048 nodes a workgroup covers" in err()
    assert _plan(0, (2049, 2049), (4098, 2049), 1, 1, 2049, 2, True, 0, 0)[0] == 0
    assert _plan(0, (2048, 2048), (4096, 2048), 1, 1, 2048, 2, False, 1, 0) == (0, (mr.SCALAR, 8, 1, 1, 1), 4 * (4 * 2048 + 2 * 2048))
    # LDS over 160 KiB: one row of 4096 nodes and 40 edges per node
    assert _plan(0, (4096, 4096), (8192, 4096), 1, 1, 4096, 40, True, 0, 0)[0] == -1
    assert b"mrconv_fwd: N=4096 K=40 needs 671744 B of LDS (> 160 KiB)" in err()
    assert _plan(0, (1024, 1024), (2048, 1024), 1, 1, 1024, 40, True, 1, 0)[0] == -1
    assert b"mrconv_bwd: N=1024 K=40 needs 180224 B of LDS (> 160 KiB)" in err()
    # arguments
    assert lib.grafp_mrconv_plan(0, 64, 64, 128, 64, 1, 1, 64, 3, 1, 0, 0, None) == -1 and b"mrconv_plan: null pointer" in err()
    assert lib.grafp_mrconv_plan(0, 64, 64, 128, 64, 1, 1, 64, 0, 1, 0, 0, info) == -1 and b"bad shape" in err()
    assert lib.grafp_mrconv_plan(7, 64, 64, 128, 64, 1, 1, 64, 3, 1, 0, 0, info) == -1 and b"dtype" in err()
