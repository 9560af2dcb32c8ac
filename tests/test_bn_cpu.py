"""CPU tests of the BatchNorm reference the GPU tests compare bn.hip with (tests/_bn_ref.py): its plain formulas against
float64 F.batch_norm + autograd run view by view, and the properties of the case table the GPU bars rely on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bn_ref as br


def _torch_views(case, i):
    """The case through torch in float64: one F.batch_norm call per view, in view order, on shared running statistics."""
    d = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float64))          # noqa: E731
    C, G, Mg = case.C, case.G, case.Mg
    x = d(i["x"]).requires_grad_(True)
    gamma, beta = d(i["gamma"]).requires_grad_(True), d(i["beta"]).requires_grad_(True)
    pb = d(i["pb"]).requires_grad_(True) if case.pb else None
    res = d(i["res"]).requires_grad_(True) if case.res else None
    rm, rv = d(i["rm0"]).clone(), d(i["rv0"]).clone()
    outs, pres = [], []
    for g in range(G):
        xv = x[:, g * Mg:(g + 1) * Mg]
        if pb is not None:
            xv = xv + pb[:, None]
        y = F.batch_norm(xv.reshape(1, C, Mg), rm, rv, gamma, beta, case.training, br.MOMENTUM, br.EPS).reshape(C, Mg)
        pres.append(y)
        z = F.relu(y) if case.act == br.ACT_RELU else (F.leaky_relu(y, br.SLOPE) if case.act == br.ACT_LEAKY else y)
        outs.append(z if res is None else z + res[:, g * Mg:(g + 1) * Mg])
    out = torch.cat(outs, dim=1)
    out.backward(d(i["dz"]))
    grad = lambda t: None if t is None else t.grad.numpy()                                          # noqa: E731
    return dict(out=out.detach().numpy(), pre=torch.cat(pres, dim=1).detach().numpy(), rm=rm.numpy(), rv=rv.numpy(),
                dx=grad(x), dgamma=grad(gamma), dbeta=grad(beta), dpb=grad(pb), dres=grad(res))


@pytest.mark.parametrize("name", br.SMALL_CASES)
def test_reference_formulas_equal_torch_float64(name):
    """Both sides are float64, so they agree to rounding: 1e-11 of each result's largest entry (the constant row divides
    by sqrt(eps), which amplifies the last bits of dy - mean(dy) by 316)."""
    case = br.CASE_BY_NAME[name]
    inputs, ref = br.cached_case(name)
    want = _torch_views(case, inputs)
    for key, w in want.items():
        if w is None:
            assert ref[key] is None, key
            continue
        got = np.asarray(ref[key], dtype=np.float64)
        assert got.shape == w.shape, key
        # (autograd's dpre_bias is the sum of a row of dx, exactly zero only in exact arithmetic: its scale is sum |dx|)
        scale = float(np.abs(want["dx"]).sum(axis=1).max()) if key == "dpb" else max(float(np.max(np.abs(w))), 1.0)
        assert float(np.max(np.abs(got - w))) <= 1e-11 * scale, key
    if case.training:
        assert not np.any(ref["dpb"]) if case.pb else ref["dpb"] is None
    else:
        assert np.array_equal(ref["rm"], inputs["rm0"].astype(np.float64))
        assert np.array_equal(ref["rv"], inputs["rv0"].astype(np.float64))


@pytest.mark.parametrize("name", [c.name for c in br.CASES])
def test_case_inputs_and_ambiguous_relu_positions(name):
    """Every case: at most 0.1 % of the elements have a float64 pre-activation within the f32 output bar of zero (they
    leave the dx comparison and widen the dgamma / dbeta bars); row 0 has |mean| = 30 std, row 2 is constant at 3.0; bf16
    inputs are bf16 values."""
    case = br.CASE_BY_NAME[name]
    inputs, ref = br.cached_case(name)
    amb = br.ambiguous(case, ref)
    assert amb.mean() <= 1e-3, (int(amb.sum()), amb.size)
    x = inputs["x"].astype(np.float64)
    ratio = abs(x[0].mean()) / x[0].std()                 # (a sample of 7 or 256 columns has no exact std)
    assert abs(ratio - 30.0) < 1.5 if case.Mg >= 1000 else ratio > 20.0
    if case.C >= 3:
        assert np.all(inputs["x"][2] == 3.0)
    if case.dt == "bf16":
        for key in ("x", "dz", "res"):
            if inputs[key] is not None:
                assert np.array_equal(br.bf16_round(inputs[key]), inputs[key]), key


def test_case_table_covers_every_path_dtype_and_view_count():
    """Path code x dtype x {1, > 1 views}, every activation and pre_bias present / absent on every path, and the plan
    each case expects is consistent with its shape."""
    seen, acts, pbs = set(), set(), set()
    for c in br.CASES:
        for path in (c.fwd[0], c.bwd[0]):
            seen.add((path, c.dt, c.G > 1))
            acts.add((path, c.act))
            pbs.add((path, c.pb))
        W = 4 if c.dt == "f32" else 8
        for path, items, threads, chunks in (c.fwd, c.bwd):
            if path == br.PATH_1PASS:
                assert c.training and not c.two_pass and c.Mg % W == 0 and chunks * c.G <= 256
                assert chunks == -(-c.Mg // (threads * items * W))
            if path == br.PATH_2PASS_VEC:
                assert c.Mg % W == 0
    assert seen == {(p, dt, v) for p in (0, 1, 2) for dt in ("f32", "bf16") for v in (False, True)}
    assert acts == {(p, a) for p in (0, 1, 2) for a in (0, 1, 2)}
    assert pbs == {(p, b) for p in (0, 1, 2) for b in (False, True)}
    assert len(br.CASE_BY_NAME) == len(br.CASES)


def test_reference_keeps_nan_and_inf_like_torch():
    """One NaN, and one +Inf, in a training row: the whole view comes out NaN in the output and in dx (ReLU included),
    running_var is NaN, running_mean is NaN / +Inf; in eval mode only the poisoned position of the output is NaN."""
    case = br.CASE_BY_NAME["f32-sc-1001-3v"]
    inputs, _ = br.cached_case(case.name)
    for poison in (np.nan, np.inf):
        for act in (0, 1, 2):
            for training in (True, False):
                i = dict(inputs)
                i["x"] = inputs["x"].copy()
                i["x"][1, case.Mg + 5] = poison
                r = br.bn_ref(i["x"], i["dz"], i["res"], i["gamma"], i["beta"], i["pb"], i["rm0"], i["rv0"], case.G, act, training)
                want = np.zeros(i["x"].shape, bool)
                if training:
                    want[1, case.Mg:2 * case.Mg] = True
                    assert np.array_equal(np.isnan(r["dx"]), want)
                    assert np.isnan(r["rv"][1]) and not np.isnan(r["rv"][0])
                    assert np.isnan(r["rm"][1]) if np.isnan(poison) else r["rm"][1] == np.inf
                else:
                    want[1, case.Mg + 5] = bool(np.isnan(poison))
                    assert not np.isnan(r["dx"]).any()
                assert np.array_equal(np.isnan(r["out"]), want), (poison, act, training)


@pytest.mark.parametrize("name", [c.name for c in br.CASES if c.Mg >= br.LONG_ROW])
def test_long_row_float32_error_is_reported(name):
    """Rows of 2^16 columns and more: prints the float32-formula error the GPU bars are derived from (pytest -s)."""
    case = br.CASE_BY_NAME[name]
    inputs, ref = br.cached_case(name)
    err = br.long_row_error(case, inputs, ref)
    b, _ = br.bars(case, ref)
    for key, e in err.items():
        print(f"long-row {name} {key}: f32-vs-f64 {e:.3e}  x16 {16 * e:.3e}  f32 bar (largest) {float(np.max(b[key])):.3e}")
        assert np.isfinite(e)


def test_plan_query_reports_the_hand_derived_launches():
    """grafp_bn_plan is a pure host function: every case's expected launch (worked out by hand in the table) is what the
    library reports for it, and bad arguments are refused with a message."""
    import ctypes
    from grafp_amd._lib import lib
    info = (ctypes.c_int * 8)()
    for c in br.CASES:
        fwd_aligned, bwd_aligned = c.misalign not in ("x", "res"), c.misalign not in ("x", "dz")
        for backward, aligned, want in ((0, fwd_aligned, c.fwd), (1, bwd_aligned, c.bwd)):
            assert lib.grafp_bn_plan(0 if c.dt == "f32" else 1, c.C, c.Mg * c.G, c.G, int(c.training), backward,
                                     int(aligned), int(not c.two_pass), info) == 0
            assert tuple(info[:4]) == want, (c.name, backward, tuple(info[:5]))
            assert info[3] == -(-c.Mg // info[4]) and list(info[5:8]) == [0, 0, 0]
    assert lib.grafp_bn_plan(0, 4, 1024, 1, 1, 0, 1, 1, None) == -1 and b"null pointer" in lib.grafp_last_error()
    assert lib.grafp_bn_plan(0, 4, 1023, 2, 1, 0, 1, 1, info) == -1 and b"groups" in lib.grafp_last_error()
    assert lib.grafp_bn_plan(7, 4, 1024, 1, 1, 0, 1, 1, info) == -1 and b"dtype" in lib.grafp_last_error()
