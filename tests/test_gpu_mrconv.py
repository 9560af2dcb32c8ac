"""GPU tests of the max-relative kernels (grafp_amd/csrc/mrconv.hip) on every launch path: each case asserts through
grafp_mrconv_plan which kernel it runs, with the pointers it actually passes, then compares the output and dx with the
numpy reference of tests/_mrconv_ref.py -- exactly (torch.equal): the inputs are chosen so that the exact result is
representable (see that file).  f32 and bf16, (B, C, N) and (C, B, N).  `pytest -m gpu` on an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

import _mrconv_ref as mr

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def _plan(t, x_s, o_s, B, C, N, K, backward, with_arg, *tensors):
    """info[:5] of grafp_mrconv_plan for a call on these activation tensors (their real alignment)."""
    from grafp_amd import ops
    info = (ctypes.c_int * 8)()
    aligned = all(a.data_ptr() % (4 * a.element_size()) == 0 for a in tensors)
    ops.check(ops.lib.grafp_mrconv_plan(ops._DT[t], x_s[0], x_s[1], o_s[0], o_s[1], B, C, N, K, int(aligned), int(backward),
                                        int(with_arg), info), "mrconv_plan")
    return tuple(info[:5])


def _to_dev(a, dt, layout, dev, off1=False):
    """(B, C, N) -> device tensor of dtype dt in the layout; off1: a contiguous view at storage offset 1 of a larger buffer."""
    t = torch.tensor(a).to(dev).to(DT[dt])
    if layout == "cbn":
        t = t.permute(1, 0, 2).contiguous()
    if not off1:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() == 1 and view.data_ptr() % (4 * view.element_size()) != 0
    return view


def _run(dev, monkeypatch, dt, layout, record, x, idx, g, idx32=False, off1=False):
    """One forward + backward of ops.max_relative; out and dx come back on the device in (B, C, N) order, with the
    (forward, backward) launches grafp_mrconv_plan reports for the pointers that were passed."""
    from grafp_amd import ops
    monkeypatch.setattr(ops.switches, "mrconv_arg", bool(record))
    B, C, N = x.shape
    K = idx.shape[-1]
    xg = _to_dev(x, dt, layout, dev, off1).requires_grad_(True)
    gg = _to_dev(g, dt, layout, dev)
    ig = torch.tensor(idx).to(dev).to(torch.int32 if idx32 else torch.int64)
    out = ops.max_relative(xg, ig, layout=layout)
    seen = []
    out.register_hook(lambda t: seen.append(t.data_ptr()))
    out.backward(gg)
    torch.cuda.synchronize()
    assert seen == [gg.data_ptr()], "autograd handed the backward another gradient buffer than the test built"
    assert out.dtype == DT[dt] and xg.grad.dtype == DT[dt] and xg.grad.shape == xg.shape
    x_s, o_s = ((C * N, N), (2 * C * N, N)) if layout == "bcn" else ((N, B * N), (N, B * N))
    fwd = _plan(DT[dt], x_s, o_s, B, C, N, K, False, record, xg, out)
    from_record = record and fwd[0] == mr.RECORD
    bwd = _plan(DT[dt], x_s, o_s, B, C, N, K, True, from_record, *((gg, xg.grad) if from_record else (xg, gg, xg.grad)))
    bcn = lambda t: t.detach() if layout == "bcn" else t.detach().permute(1, 0, 2)              # noqa: E731
    return bcn(out), bcn(xg.grad), (fwd, bwd)


_WANT = {}


def _want(name, dt, dev):
    """The reference of a case on the device in dtype dt: computed once per case, uploaded once per (case, dtype).  The f32
    reference is exact and within bf16's range, so its bf16 form is the exact result rounded once."""
    if (name, dt) not in _WANT:
        _, (out, dx) = mr.cached_case(name)
        _WANT[name, dt] = (torch.tensor(out).to(dev).to(DT[dt]), torch.tensor(dx).to(dev).to(DT[dt]))
    return _WANT[name, dt]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in mr.CASES])
def test_max_relative_equals_the_reference_on_every_path(dev, monkeypatch, name, dt):
    """Every row of the case table, both layouts; the rows whose shape has an arg-max record run once with it (forward
    <WK>, backward from the record) and once without (the persistent recomputing backward), the others with the switch
    as it is by default -- where `scalar-by-pointer` requires a gradient on a misaligned x and must take the scalar kernels.
    Output and dx are the reference's, bit for bit."""
    case = mr.CASE_BY_NAME[name]
    (x, idx, g), _ = mr.cached_case(name)
    mr.check_grid(case, g)
    want_out, want_dx = _want(name, dt, dev)
    for layout in ("bcn", "cbn"):
        for record in ((True, False) if case.rec else (True,)):
            out, dx, plans = _run(dev, monkeypatch, dt, layout, record, x, idx, g, case.idx32, case.off1)
            print(f"mrconv-plan {name} {dt} {layout} record={record}: fwd {plans[0]} bwd {plans[1]}")
            assert plans == (case.rec if record and case.rec else (case.fwd, case.bwd)), plans
            assert torch.equal(out, want_out), (layout, record, "out", int((out != want_out).sum()))
            assert torch.equal(dx, want_dx), (layout, record, "dx", int((dx != want_dx).sum()))


def _disputed_and_reference(x, idx, g):
    """x[edge 0] - x and x[later edges] - x of every (clip, channel, node), and the reference's dx."""
    B, C, _ = x.shape
    bi, ci = np.arange(B)[:, None, None], np.arange(C)[None, :, None]
    first = x[bi, ci, idx[:, None, :, 0]] - x
    rest = x[bi[..., None], ci[..., None], idx[:, None, :, 1:]] - x[..., None]
    return first, rest, mr.mr_ref(x, idx, g, winner_of=mr.first_max_edge)[1]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_first_maximum_is_one_rule_on_every_path(dev, monkeypatch, dt):
    """Edge 0 is NOT the node itself here, and x is NaN at some nodes, +inf at others: for a node whose edge 0 leads to a
    NaN -- or from +inf to +inf, whose difference is NaN -- the first maximum is edge 0, as torch.max returns the first NaN.
    (A NaN on a LATER edge never wins on any path, `v > best` being false: there torch.max differs, and the reference
    here is the rule itself, tests/_mrconv_ref.py first_max_edge.)  The record path, the persistent recomputing backward
    and the generic scalar kernels (x at storage offset 1) route alike: the same dx bits, and the rule's.
    The gradients stay finite, so no slab is poisoned: a non-finite gradient turns the dx of its whole SLAB into NaN, and a
    slab is 2 rows here on the persistent paths and 8 on the scalar one, so how far that reaches is not comparable across
    paths and not tested across them."""
    case = mr.CASE_BY_NAME["scalar-by-pointer"]
    B, N = case.B, case.N
    x, idx, g = (a.copy() for a in mr.case_inputs(case))
    idx[:, :, 0] = (np.arange(N)[None, :] + 1 + 3 * np.arange(B)[:, None]) % N
    x[0, 1, 5] = x[1, 2, 40] = x[1, 2, 41] = np.nan
    x[0, 3, 9] = x[0, 3, 10] = x[1, 7, 63] = np.inf                 # node 9 -> edge 0 = node 10: inf - inf
    with np.errstate(invalid="ignore"):                             # inf - inf, on purpose
        first, rest, want_dx = _disputed_and_reference(x, idx, g)
    disputed = np.isnan(first) & ~np.isnan(rest).all(axis=-1)
    assert disputed.sum() >= 4, "no node whose edge 0 is NaN while a later edge is not: the rule is not exercised"
    assert np.isfinite(want_dx).all()
    want_dx = torch.tensor(want_dx).to(dev).to(DT[dt])
    runs = {"record": (True, False, (mr.RECORD, mr.RECORD)), "persistent": (False, False, (mr.PERSISTENT, mr.PERSISTENT)),
            "scalar": (True, True, (mr.SCALAR, mr.SCALAR))}
    got = {}
    for what, (record, off1, paths) in runs.items():
        out, dx, plans = _run(dev, monkeypatch, dt, "bcn", record, x, idx, g, False, off1)
        assert (plans[0][0], plans[1][0]) == paths, (what, plans)
        got[what] = (out.nan_to_num(7.0), dx.nan_to_num(7.0))
        assert torch.equal(dx, want_dx), (what, int((dx != want_dx).sum()))
    for what in ("persistent", "scalar"):
        assert torch.equal(got[what][0], got["record"][0]), what
        assert torch.equal(got[what][1], got["record"][1]), what
