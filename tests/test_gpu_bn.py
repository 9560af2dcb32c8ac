"""GPU tests of the BatchNorm kernels (grafp_amd/csrc/bn.hip) on every launch path: each case asserts through
grafp_bn_plan which kernel variant it runs, then compares forward, saved and running statistics and every gradient with
the float64 reference of tests/_bn_ref.py; non-finite inputs must come out where the reference puts them.
`pytest -m gpu` on an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

import _bn_ref as br

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def _plan(dt, C, M, G, training, backward, aligned, have_sync):
    from grafp_amd import ops
    info = (ctypes.c_int * 8)()
    ops.check(ops.lib.grafp_bn_plan(ops._DT[DT[dt]], C, M, G, int(training), int(backward), int(aligned), int(have_sync),
                                    info), "bn_plan")
    return tuple(info[:5])


def _to_dev(a, dt, dev, off1=False):
    """numpy float32 -> device tensor of the case's dtype; off1: a contiguous view at storage offset 1 of a larger buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DT[dt])
    if not off1:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() == 1 and view.data_ptr() % 16 != 0
    return view


def _run(case, inputs, dev, monkeypatch, x=None):
    """One forward + backward of ops.bn_act on the case; returns the results as float64 numpy arrays plus the launches
    grafp_bn_plan reports for the pointers that were actually passed."""
    from grafp_amd import ops
    monkeypatch.setattr(ops.switches, "bn_two_pass", bool(case.two_pass))
    M = case.Mg * case.G
    xg = _to_dev(inputs["x"] if x is None else x, case.dt, dev, case.misalign == "x").requires_grad_(True)
    gz = _to_dev(inputs["dz"], case.dt, dev, case.misalign == "dz")
    rg = _to_dev(inputs["res"], case.dt, dev, case.misalign == "res").requires_grad_(True) if case.res else None
    f = lambda a: torch.from_numpy(a).to(dev)                                        # noqa: E731
    gg, bg = f(inputs["gamma"]).requires_grad_(True), f(inputs["beta"]).requires_grad_(True)
    pg = f(inputs["pb"]).requires_grad_(True) if case.pb else None
    rm, rv = f(inputs["rm0"]).clone(), f(inputs["rv0"]).clone()
    out = ops.bn_act(xg, gg, bg, rm, rv, case.training, br.MOMENTUM, br.EPS, pg, rg, case.act, br.SLOPE, case.G)
    seen = []
    out.register_hook(lambda g: seen.append(g.data_ptr()))
    out.backward(gz)
    torch.cuda.synchronize()
    assert seen == [gz.data_ptr()], "autograd handed the backward another dz buffer than the test built"
    assert out.dtype == DT[case.dt] and xg.grad.dtype == DT[case.dt]
    have_sync = not case.two_pass
    al = lambda *ts: all(t is None or t.data_ptr() % 16 == 0 for t in ts)              # noqa: E731
    plans = (_plan(case.dt, case.C, M, case.G, case.training, False, al(xg, out, rg), have_sync),
             _plan(case.dt, case.C, M, case.G, case.training, True, al(xg, gz, xg.grad), have_sync))
    n = lambda t: None if t is None else t.detach().double().cpu().numpy()              # noqa: E731
    got = dict(out=n(out), dx=n(xg.grad), dgamma=n(gg.grad), dbeta=n(bg.grad), rm=n(rm), rv=n(rv),
               dpb=n(pg.grad) if case.pb else None, dres=n(rg.grad) if case.res else None)
    if any(p[0] == br.PATH_1PASS for p in plans):
        for buf in ops._BN_SYNC.values():
            assert bool((buf == -1).all()), "rendezvous buffer not re-armed"
    return got, plans


def _saved_stats(case, inputs, dev, monkeypatch):
    """save_mean / save_invstd of the forward launch (the autograd function keeps them to itself): the same call through
    the C entry, with the pointers aligned as the case has them."""
    from grafp_amd import ops
    monkeypatch.setattr(ops.switches, "bn_two_pass", bool(case.two_pass))
    C, M = case.C, case.Mg * case.G
    x = _to_dev(inputs["x"], case.dt, dev, case.misalign == "x")
    res = _to_dev(inputs["res"], case.dt, dev, case.misalign == "res") if case.res else None
    f = lambda a: None if a is None else torch.from_numpy(a).to(dev)                  # noqa: E731
    gamma, beta, pb, rm, rv = (f(inputs[k]) for k in ("gamma", "beta", "pb", "rm0", "rv0"))
    out = torch.empty_like(x)
    mean = torch.empty((C, case.G), dtype=torch.float32, device=dev)
    invstd = torch.empty((C, case.G), dtype=torch.float32, device=dev)
    nbytes = ops.lib.grafp_bn_workspace(C, M)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    p = ops._p
    ops.check(ops.lib.grafp_bn_fwd_1pass(p(x), ops._DT[x.dtype], C, M, case.G, p(pb), p(gamma), p(beta), p(res), case.act,
                                         br.SLOPE, br.EPS, br.MOMENTUM, int(case.training), p(rm), p(rv), p(out), p(mean),
                                         p(invstd), p(ws), nbytes, p(ops._bn_sync(x.device, C, M)), -1, ops._stream()), "bn_fwd")
    torch.cuda.synchronize()
    return mean.double().cpu().numpy(), invstd.double().cpu().numpy(), out.double().cpu().numpy()


def _worst(got, want, bar, keep=None):
    """max over the compared positions of |got - want| / bar (<= 1 passes) and the largest |got - want|."""
    d = np.abs(np.asarray(got, np.float64) - want)
    q = d / bar
    if keep is not None:
        d, q = d[keep], q[keep]
    return (float(q.max()), float(d.max())) if q.size else (0.0, 0.0)


@pytest.mark.parametrize("name", [c.name for c in br.CASES])
def test_bn_vs_float64_on_every_path(dev, monkeypatch, name):
    """Every kernel variant of bn.hip against float64 (tests/_bn_ref.py; bf16 from the widened bf16 values).
    Bars: f32 -- out 2e-5 rel + abs, gradients 1e-4 rel + 1e-4 max|ref|, running / saved mean 1e-5, running var and
    invstd 1e-4 rel + 1e-5 (those of test_bn_act_forward_backward_f32); bf16 out and dx add one rounding, 2^-8 |ref|;
    positions whose float64 pre-activation is within the out bar of zero leave the dx comparison and add their |dz|,
    |dz xhat| to the dbeta, dgamma bars.  dpre_bias is exactly 0 in training mode; the residual's gradient is dz itself.
    Rows of >= 2^16 columns per view take 16 x the error of the same formulas in numpy float32 against float64 where
    that exceeds the f32 bar.  Measured (float32 error -> 16 x; it exceeds the f32 bar only for `out` of f32-over256,
    1.333e-04 against 6.3e-05):
      bf16-1p-i8          out 5.688e-06 -> 9.101e-05   dx 1.518e-07 -> 2.429e-06   dgamma 1.049e-03 -> 1.678e-02
      bf16-1p-i8-t512-2v  out 7.565e-07 -> 1.210e-05   dx 1.016e-07 -> 1.625e-06   dgamma 1.992e-04 -> 3.187e-03
      f32-over256         out 8.329e-06 -> 1.333e-04   dx 2.121e-07 -> 3.394e-06   dgamma 3.029e-03 -> 4.846e-02
      bf16-over256        out 9.438e-06 -> 1.510e-04   dx 2.205e-07 -> 3.528e-06   dgamma 6.013e-02 -> 9.620e-01
    The row constant at 3.0 is what found the forward's folded offset (bn.hip, BnNorm): with beta + (pb - mean) g rounded
    at |3 g| = 949 the output of that row missed float64 by 9.4e-5 (f32-1p-4096-3v) and 5.4e-5 (f32-sc-7) against a bar
    of 2.2e-5; rows that far from zero now subtract the mean first."""
    case = br.CASE_BY_NAME[name]
    inputs, ref = br.cached_case(name)
    got, (fwd, bwd) = _run(case, inputs, dev, monkeypatch)
    print(f"bn-plan {name}: fwd {fwd} bwd {bwd}")
    assert fwd[:4] == case.fwd and bwd[:4] == case.bwd, (fwd, bwd)
    bar, amb = br.bars(case, ref, br.long_row_error(case, inputs, ref))
    mean, invstd, out2 = _saved_stats(case, inputs, dev, monkeypatch)
    assert np.array_equal(out2, got["out"])                          # the direct call is the launch the autograd call made
    got["mean"], got["invstd"] = mean, invstd
    worst = {}
    for key in ("out", "mean", "invstd", "rm", "rv", "dx", "dgamma", "dbeta"):
        assert np.isfinite(got[key]).all(), key
        worst[key] = _worst(got[key], ref[key], bar[key], ~amb if key == "dx" else None)
    print(f"bn-err {name}: " + "  ".join(f"{k} {q:.3f} ({d:.3e})" for k, (q, d) in worst.items()))
    if case.pb:
        if case.training:
            assert not got["dpb"].any()
        else:
            tol = 1e-4 * np.abs(ref["dpb"]) + 1e-4 * float(np.abs(ref["dpb"]).max())
            assert (np.abs(got["dpb"] - ref["dpb"]) <= tol).all()
    if case.res:
        assert np.array_equal(got["dres"], inputs["dz"].astype(np.float64))
    if not case.training:
        assert np.array_equal(got["rm"], inputs["rm0"].astype(np.float64))
        assert np.array_equal(got["rv"], inputs["rv0"].astype(np.float64))
    for key, (q, d) in worst.items():
        where = np.unravel_index(int(np.argmax(np.abs(got[key] - ref[key]) / bar[key])), np.shape(ref[key]))
        assert q <= 1.0, (key, q, d, "row", int(where[0]))


# ---- the recompute fallback of the single-pass rendezvous ----------------------------------------------------------------
_ONE_PASS = [c.name for c in br.CASES if br.PATH_1PASS in (c.fwd[0], c.bwd[0])]


def _bits(a):
    # float64 widened exactly from f32 / bf16: equal bits here are equal bits there (-0.0 and NaN payloads included)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", _ONE_PASS)
def test_bn_single_pass_recompute_gives_the_same_bits(dev, monkeypatch, name):
    """Every case of the table with a single-pass launch (f32 and bf16; 4 / 256, 8 / 256 and 8 / 512; ragged last chunks;
    one, two and three views), once as is and once with a spin limit of 0, where a workgroup does not wait but recomputes
    from the row whatever partial sums are not yet published: all results are the same bits, and the rendezvous buffer is
    all ones again afterwards."""
    from grafp_amd import ops
    case = br.CASE_BY_NAME[name]
    inputs = br.case_inputs(case)
    want, plans = _run(case, inputs, dev, monkeypatch)
    assert (plans[0][:4], plans[1][:4]) == (case.fwd, case.bwd), plans
    monkeypatch.setattr(ops.switches, "bn_spin_limit", 0)
    got, _ = _run(case, inputs, dev, monkeypatch)
    for key in ("out", "dx", "dgamma", "dbeta", "rm", "rv"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key
    assert ops._BN_SYNC
    for buf in ops._BN_SYNC.values():
        assert bool((buf == -1).all()), "rendezvous buffer not re-armed"


# ---- non-finite inputs ------------------------------------------------------------------------------------------------
_POISON_MODES = {"single-pass": (True, False), "two-pass": (True, True), "eval": (False, False)}


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("mode", list(_POISON_MODES))
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bn_non_finite_input_comes_out_where_float64_puts_it(dev, monkeypatch, dt, mode, poison):
    """One NaN / one +Inf in view 1 of row 1 (3 rows, 2 views of 4096 columns), every activation: the NaN positions of
    the output, dx and the running statistics are the float64 reference's -- a training view with a poisoned element is
    NaN throughout (its mean or variance is), in eval mode only a NaN element itself is -- and rows 0 and 2 are
    bit-identical to the run without the poison."""
    training, two_pass = _POISON_MODES[mode]
    for act in (br.ACT_NONE, br.ACT_RELU, br.ACT_LEAKY):
        case = br.Case(f"poison-{dt}-{mode}", dt, 3, 4096, 2, act, True, True, training, two_pass, None, None, None)
        inputs = br.case_inputs(case)
        clean, plans = _run(case, inputs, dev, monkeypatch)
        want_path = br.PATH_1PASS if mode == "single-pass" else br.PATH_2PASS_VEC
        assert plans[0][0] == want_path and plans[1][0] == want_path, plans
        x = inputs["x"].copy()
        x[1, case.Mg + 1234] = poison
        ref = br.bn_ref(x, inputs["dz"], inputs["res"], inputs["gamma"], inputs["beta"], inputs["pb"], inputs["rm0"],
                        inputs["rv0"], case.G, act, training)
        got, _ = _run(case, inputs, dev, monkeypatch, x=x)
        for key in ("out", "dx", "rm", "rv"):
            assert np.array_equal(np.isnan(got[key]), np.isnan(ref[key])), \
                (act, key, int(np.isnan(got[key]).sum()), int(np.isnan(ref[key]).sum()))
        for key in ("out", "dx", "rm", "rv", "dgamma", "dbeta"):
            assert np.array_equal(got[key][[0, 2]], clean[key][[0, 2]]), (act, key)


def _bf16(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(dev)


def _nan_columns(t):
    return torch.isnan(t.float()).cpu().numpy()


@pytest.mark.parametrize("act", [0, 1, 2])
def test_affine_and_normalise_on_load_keep_nan(dev, act):
    """The other places a BatchNorm's activation is applied -- bn_affine, the affine epilogue of conv1x1_gemm_affine, the
    normalise-on-load operand of conv1x1_gemm and of the weight gradient (smallest shapes gemm_supported accepts: 32 x 32
    weights, 128 columns per view, 2 views): a NaN goes where float64 arithmetic puts it, everything else is bit-identical
    to the clean run; a +Inf makes no NaN in the elementwise forms."""
    from grafp_amd import ops
    from _hashfill import hash_normalish, hash_uniform
    R = K = 32
    views, Mg = 2, 128
    M = views * Mg
    assert ops.gemm_supported(R, K, 1, M, views)
    w = _bf16(0.2 * hash_normalish("bn:nan.w", (R, K)), dev)
    x_np = br.bf16_round(hash_normalish("bn:nan.x", (K, M)))
    g = _bf16(hash_normalish("bn:nan.g", (R, M)), dev)
    scale = 0.75 + 0.25 * hash_uniform("bn:nan.s", (R, views))              # > 0: a +Inf stays +Inf
    tab = torch.from_numpy(np.stack((scale, hash_uniform("bn:nan.t", (R, views))), axis=-1)).to(dev)
    row, col = 5, Mg + 17
    for poison in (float("nan"), float("inf")):
        xp_np = x_np.copy()
        xp_np[row, col] = poison
        x, xp = _bf16(x_np, dev), _bf16(xp_np, dev)
        isnan = np.isnan(poison)
        # -- bn_affine: elementwise, so only the element itself
        clean, got = ops.bn_affine(x, tab, views, act=act, slope=0.2), ops.bn_affine(xp, tab, views, act=act, slope=0.2)
        want = np.zeros((K, M), bool)
        want[row, col] = isnan
        assert np.array_equal(_nan_columns(got), want), ("bn_affine", poison)
        keep = torch.ones(K, dtype=torch.bool)
        keep[row] = False
        assert torch.equal(got[keep], clean[keep])
        # -- products: the poisoned operand element reaches every output row of its column (0.2 * normal weights: none is 0)
        colmask = np.zeros((R, M), bool)
        colmask[:, col] = True
        others = torch.from_numpy(~colmask[0]).to(dev)
        for what, run in (("gemm_affine", lambda xx: ops.conv1x1_gemm_affine(w, xx, tab, 1, views, act=act, slope=0.2)),
                          ("gemm_pro", lambda xx: ops.conv1x1_gemm(w, xx, 1, views, pro_tab=tab, pro_act=act, pro_slope=0.2))):
            clean, got = run(x), run(xp)
            if isnan:
                assert np.array_equal(_nan_columns(got), colmask), (what, poison)
            elif what == "gemm_pro":
                # f(+Inf) = +Inf for every activation (scale > 0): the column is +-Inf by the weight's sign, never NaN
                assert not _nan_columns(got).any() and bool(torch.isinf(got[:, col].float()).all())
            assert torch.equal(got[:, others], clean[:, others]), what
        # -- weight gradient with the normalise-on-load operand: dW[:, k] of the poisoned operand row k
        run = lambda xx: ops.conv1x1_wgrad(g, xx, R, K, 1, M, views, tab, act, 0.2)         # noqa: E731
        clean, got = run(x), run(xp)
        if isnan:
            want = np.zeros((R, K), bool)
            want[:, row] = True
            assert np.array_equal(_nan_columns(got), want), ("wgrad_pro", poison)
        keepk = torch.ones(K, dtype=torch.bool)
        keepk[row] = False
        assert torch.equal(got[:, keepk], clean[:, keepk])
