"""GPU tests of the fused layer ops.conv_bn_act (_ConvBnAct: forward and backward) and of the residual block built from
it -- ShortcutToken, DeferredNorm, prepared weights, a derived weight -- against the float64 autograd reference of
tests/_layer_ref.py, on every tile configuration gemm_plan can choose for the forward, the data-gradient and the
concatenated-operand product.  `pytest -m gpu tests/test_gpu_layer.py` on an MI355X.

The reference takes the layer's own y (the tensor its backward pass will read, from z.grad_fn.saved_tensors) after y
was checked against the float64 product with the bars of test_gpu_gemm.py; everything downstream is float64 on those
bits.  Every comparison asserts, per output, the per-element bar of _layer_ref.BARS outside the disputed positions and
the relative-L2 ceiling of test_gpu_bf16_backward.py (5e-3 activations, 7e-3 parameters) over the whole tensor, and
prints the worst per-element value and the relative L2 of every output.

Measured on the MI355X (`pytest -m gpu tests/test_gpu_layer.py -s`, which prints one line per comparison): the worst
per-element deviation per case and output over every option that runs the case -- bf16 outputs (z, dx, dres) in rounding
steps |got - want| / (2^-8 max(|want|, row RMS of want)), f32 outputs as |got - want| / max |want| -- outside the disputed
positions (none arose: every line printed `disputed 0`).  The bars of _layer_ref.BARS are twice these values, bf16 ones
rounded up to whole steps, f32 ones rounded up to two digits; zero where bit equality was measured.  The block rows
are the worst over fused / accumulated shortcut, prepared / on-the-fly operands, deferred / separate normalisation; dx
of a block reaches 2.9 steps only where autograd accumulates the shortcut (two roundings), 2.0 through [W^T | I].
  tiny          z 0.419  dx 1.54  dw 0.000128  dgamma 1.6e-07  dbeta 8.55e-08  dpb 9.5e-08  dres 0  rm 2.36e-07  rv 1.09e-07
  large         z 1.3  dx 1.64  dw 9.31e-05  dgamma 1.59e-07  dbeta 7.43e-08  dpb 0  dres 0  rm 1.24e-07  rv 1.48e-07
  xl            z 1.05  dx 1.92  dw 3.84e-05  dgamma 1.28e-07  dbeta 8.71e-08  dpb 1.81e-07  dres 0  rm 4.72e-08  rv 7.75e-08
  n32           z 1.95  dx 2  dw 7.09e-05  dgamma 3.86e-07  dbeta 1.02e-07  dpb 0  dres 0  rm 1.14e-07  rv 7.95e-08
  n64           z 1.84  dx 2  dw 3.86e-05  dgamma 2.27e-07  dbeta 8.78e-08  dpb 0  dres 0  rm 1.82e-07  rv 9.87e-08
  n128          z 2  dx 2  dw 3.35e-05  dgamma 1.91e-07  dbeta 1.41e-07  dpb 0  dres 0  rm 1.48e-07  rv 7.91e-08
  grouped       z 1.83  dx 2.11  dw 0.00025  dgamma 4.57e-07  dbeta 1.04e-07  dpb 1.07e-07  dres 0  rm 6.24e-08  rv 1.92e-07
  views5        z 0.0364  dx 1.1  dw 0.00014  dgamma 1.32e-07  dbeta 1.41e-07  dpb 0  dres 0  rm 7.47e-08  rv 1.78e-07
  block tiny    z 0  dx 2  dw1 3.26e-05  dw2 1.04e-07  dgamma1 3.9e-05  dgamma2 1.14e-07  dbeta1 2.54e-05  dbeta2 1.84e-08  dpb1 0  dpb2 0  rm1 1.52e-07  rv1 1.29e-07  rm2 1.31e-07  rv2 1.04e-07
  block xl      z 0.579  dx 2  dw1 0.000531  dw2 0.000455  dgamma1 0.0004  dgamma2 9.79e-08  dbeta1 0.000472  dbeta2 2.3e-08  dpb1 0  dpb2 0  rm1 1.15e-07  rv1 6.26e-08  rm2 1.28e-07  rv2 1.2e-07
  block n64     z 1.84  dx 2.56  dw1 6.57e-05  dw2 4.32e-05  dgamma1 6.21e-05  dgamma2 1.23e-07  dbeta1 5.3e-05  dbeta2 2.19e-07  dpb1 0  dpb2 0  rm1 1.38e-07  rv1 8.72e-08  rm2 7.01e-08  rv2 7.04e-08
  block tiny-1v z 0  dx 1.98  dw1 4.74e-06  dw2 1.31e-07  dgamma1 1.2e-07  dgamma2 1.39e-07  dbeta1 1.05e-08  dbeta2 1.86e-08  dpb1 0  dpb2 0  rm1 8.9e-08  rv1 8.72e-08  rm2 1.24e-07  rv2 6.82e-08
  block n64-2v  z 1.83  dx 2.89  dw1 6.29e-05  dw2 7.67e-05  dgamma1 5.58e-05  dgamma2 1.83e-07  dbeta1 6.66e-05  dbeta2 9.14e-08  dpb1 0  dpb2 0  rm1 1.74e-07  rv1 1.56e-07  rm2 9.52e-08  rv2 1.63e-07
  worst relative L2: z 4.5e-05  dx 0.0026  dw 0.00016  dgamma 0.00016  dbeta 0.00018  dpb 1e-07  dres 0  rm 1.4e-07  rv 1.6e-07
No relative L2 comes near its ceiling (5e-3 / 7e-3): the largest is dx of a block with the accumulated shortcut, 2.6e-3.
Every planted defect of _layer_ref.DEFECTS lands at >= 54 bars (test_layer_cpu.py; the two largest cases here).
"""
import pytest
import torch

import _layer_ref as lr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACTS = [lr.ACT_NONE, lr.ACT_RELU, lr.ACT_LEAKY]
ACT_NAME = {lr.ACT_NONE: "none", lr.ACT_RELU: "relu", lr.ACT_LEAKY: "leaky"}
LARGE = 4096                          # cases with more columns assert the cap on disputed columns before they compare
_ON_DEV = {}


def _inputs(kind, name):
    if (kind, name) not in _ON_DEV:
        src = lr.case_inputs(name) if kind == "layer" else lr.block_inputs(name)
        _ON_DEV[kind, name] = {k: v.to(DEV) for k, v in src.items()}
    return _ON_DEV[kind, name]


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _check_product(y, ref64):
    """The bars of test_gpu_gemm._check_product: a bf16 result of an f32 accumulation in another order."""
    y, ref = y.float(), ref64.float().to(torch.bfloat16).float()
    tol = ref.abs() * 2.0 ** -7 + ref.abs().max() * 2.0 ** -15
    bad = (y - ref).abs() > tol
    assert not bool(bad.any()), (int(bad.sum()), float((y - ref).abs().max()))
    assert float((y != ref).float().mean()) < 5e-3


def _check_product_on_load(y, ref64):
    """The bars of test_gpu_gemm.test_gemm_normalise_on_load: an operand may have crossed a bf16 rounding boundary."""
    y, ref = y.float(), ref64.float().to(torch.bfloat16).float()
    assert float((y - ref).norm() / ref.norm()) < 2e-3
    assert float(((y - ref).abs() > ref.abs() * 2.0 ** -6 + ref.abs().max() * 2.0 ** -12).float().mean()) < 1e-3


def _compare(case, tag, got, want, M):
    bars = lr.BARS[case]
    disputed = want["disputed"]
    if M > LARGE:
        assert float(disputed.any(dim=0).double().mean()) <= lr.DISPUTED_CAP, (tag, int(disputed.sum()))
    w = lr.worst(got, want, disputed)
    print(f"{tag}: disputed {int(disputed.sum())}; " + "  ".join(f"{k} {e:.3g} (L2 {l2:.2e})" for k, (e, l2) in w.items()))
    fails = []
    for k, (e, l2) in w.items():
        b = lr.base_name(k)
        if e > bars[k]:
            fails.append((k, "per element", e, bars[k]))
        if l2 > (5e-3 if b in lr.BF16_OUT else 7e-3):
            fails.append((k, "relative L2", l2))
    assert not fails, (tag, fails)
    return w


# ------------------------------------------------------------------------------------------------
# a. one layer (b. in eval mode)
# ------------------------------------------------------------------------------------------------
def _run_layer(name, act, training=True, use_pb=True, use_res=True, grad=True):
    from grafp_amd import ops
    c, inp = lr.CASE[name], _inputs("layer", name)
    x, w, gamma, beta = _leaf(inp["x"]), _leaf(inp["w"]), _leaf(inp["gamma"]), _leaf(inp["beta"])
    pb = _leaf(inp["pb"]) if use_pb else None
    res = _leaf(inp["res"]) if use_res else None
    rm, rv = inp["rm0"].clone(), inp["rv0"].clone()
    with torch.enable_grad() if grad else torch.no_grad():
        z = ops.conv_bn_act(x, w, gamma, beta, rm, rv, training, lr.MOMENTUM, lr.EPS, pb, res, act, lr.SLOPE, c.groups, c.views)
    if not grad:
        assert z.grad_fn is None
        return dict(z=z)
    y = z.grad_fn.saved_tensors[2].detach()                   # the tensor backward will read
    assert y.shape == (c.R, c.M) and y.dtype == torch.bfloat16
    z.backward(inp["dz"])
    torch.cuda.synchronize()
    return dict(z=z.detach(), y=y, dx=x.grad, dw=w.grad, dgamma=gamma.grad, dbeta=beta.grad,
                dpb=None if pb is None else pb.grad, dres=None if res is None else res.grad, rm=rm, rv=rv)


def _layer_against_reference(name, act, training, use_pb, use_res):
    c, inp = lr.CASE[name], _inputs("layer", name)
    got = _run_layer(name, act, training, use_pb, use_res)
    _check_product(got["y"], lr._product(inp["w"].double(), inp["x"].double(), c.groups))
    want = lr.ref_layer(inp, c.groups, c.views, act, training, use_pb, use_res, y_forced=got["y"].double())
    assert torch.equal(want["y"], got["y"].double())
    tag = f"{name} {ACT_NAME[act]} {'train' if training else 'eval'} pb={int(use_pb)} res={int(use_res)}"
    _compare(name, tag, got, want, c.M)
    return got


@pytest.mark.parametrize("act", ACTS, ids=[ACT_NAME[a] for a in ACTS])
@pytest.mark.parametrize("name", [c.name for c in lr.CASES])
def test_layer_forward_and_backward_against_float64(name, act):
    """conv_bn_act in training mode, with and without a residual (on `tiny` also without pre_bias): output, dX, dW,
    dgamma, dbeta, d pre_bias, d residual and the running statistics against the reference; the forward product and the
    data gradient run on the tile configurations of the case's row (views5: finalize and affine as two launches)."""
    from grafp_amd._lib import lib
    c = lr.CASE[name]
    assert lr.plan_code(lib, c.R, c.K, c.groups, c.M, c.views) == lr.CODE[c.fwd]
    assert lr.plan_code(lib, c.K, c.R, c.groups, c.M, 1) == lr.CODE[c.dgrad]
    print(f"{name}: forward {c.fwd}, data gradient {c.dgrad}")
    for use_res in (True, False):
        for use_pb in ((True, False) if name == "tiny" else (True,)):
            _layer_against_reference(name, act, True, use_pb, use_res)


@pytest.mark.parametrize("act", [lr.ACT_RELU, lr.ACT_LEAKY], ids=["relu", "leaky"])
@pytest.mark.parametrize("name", lr.EVAL_CASES)
def test_layer_in_eval_mode(name, act):
    """Running statistics in place of batch statistics.  Under enable_grad the _ConvBnAct path: d pre_bias is not zero,
    the running statistics stay as they were; under no_grad the affine epilogue of the GEMM: the same z bits."""
    inp = _inputs("layer", name)
    for use_res in (True, False):
        got = _layer_against_reference(name, act, False, True, use_res)
        assert torch.equal(got["rm"], inp["rm0"]) and torch.equal(got["rv"], inp["rv0"])
        assert float(got["dpb"].abs().max()) > 0
    fused = _run_layer(name, act, False, True, False, grad=False)
    assert torch.equal(fused["z"], got["z"])


@pytest.mark.parametrize("name", ["tiny", "n64"])
def test_layer_backward_is_deterministic(name):
    a = _run_layer(name, lr.ACT_RELU)
    b = _run_layer(name, lr.ACT_RELU)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------
# c. the residual block with a ShortcutToken, d. with a DeferredNorm
# ------------------------------------------------------------------------------------------------
def _run_block(name, token, defer=False, prepared=False, counts=None):
    """x -> conv_bn_act (K -> H, ReLU, first layer of the block) -> conv_bn_act (H -> K, residual x, last layer), as the
    encoder's FFN calls them; token / defer: ask for a ShortcutToken / DeferredNorm through the encoder's own rules."""
    from grafp_amd import ops
    b, inp = lr.BLOCK[name], _inputs("block", name)
    x = _leaf(inp["x"])
    p = {k: _leaf(inp[k]) for k in ("gamma1", "gamma2", "beta1", "beta2", "pb1", "pb2")}
    st = {k: inp[k[:2] + "0" + k[2]].clone() for k in ("rm1", "rv1", "rm2", "rv2")}
    prep = [None, None]
    if prepared:
        convs = [torch.nn.Conv2d(b.K, b.H, 1, bias=False).to(DEV), torch.nn.Conv2d(b.H, b.K, 1, bias=False).to(DEV)]
        with torch.no_grad():
            convs[0].weight.copy_(inp["w1"].reshape(b.H, b.K, 1, 1))
            convs[1].weight.copy_(inp["w2"].reshape(b.K, b.H, 1, 1))
        convs[0]._shortcut_first = True
        owner = ops.lowp_weights(convs)
        owner.refresh(torch.bfloat16)
        prep = [cv._prepared for cv in convs]
        assert all(isinstance(pw, ops.PreparedWeight) and pw.lowp is not None and pw.owner is owner for pw in prep)
        assert prep[0].aug is not None and prep[0].t is None and prep[1].t is not None
        w1, w2 = convs[0].weight, convs[1].weight
    else:
        w1, w2 = _leaf(inp["w1"]), _leaf(inp["w2"])
    tok = ops.ShortcutToken() if token and ops.shortcut_token_supported(x) else None
    d = ops.DeferredNorm() if defer and ops.defer_norm_pays(b.K, b.H, b.M) else None
    calls = {"cat": 0, "pro": 0}
    real_cat, real_gemm = ops.conv1x1_gemm_cat, ops.conv1x1_gemm

    def cat(*a, **k):
        calls["cat"] += 1
        return real_cat(*a, **k)

    def gemm(w, x_, groups=1, views=1, pro_tab=None, pro_act=0, pro_slope=0.0, stats=False):
        calls["pro"] += pro_tab is not None
        return real_gemm(w, x_, groups, views, pro_tab, pro_act, pro_slope, stats)
    ops.conv1x1_gemm_cat, ops.conv1x1_gemm = cat, gemm
    try:
        h = ops.conv_bn_act(x, w1, p["gamma1"], p["beta1"], st["rm1"], st["rv1"], True, lr.MOMENTUM, lr.EPS, p["pb1"], None,
                            ops.ACT_RELU, 0.0, 1, b.views, prep[0], ops.LayerLinks(shortcut_in=tok, norm_out=d))
        z = ops.conv_bn_act(h, w2, p["gamma2"], p["beta2"], st["rm2"], st["rv2"], True, lr.MOMENTUM, lr.EPS, p["pb2"], x,
                            ops.ACT_NONE, 0.0, 1, b.views, prep[1], ops.LayerLinks(shortcut_out=tok, norm_in=d))
        y1, y2 = h.grad_fn.saved_tensors[2].detach(), z.grad_fn.saved_tensors[2].detach()
        z.backward(inp["dz"])
        torch.cuda.synchronize()
    finally:
        ops.conv1x1_gemm_cat, ops.conv1x1_gemm = real_cat, real_gemm
    assert tok is None or tok.grad is None                    # handed over and taken
    if counts is not None:
        counts.update(calls, token=tok is not None, deferred=d is not None)
    out = dict(z=z.detach(), y1=y1, y2=y2, h=h.detach(), dx=x.grad, dw1=w1.grad.reshape(b.H, b.K), dw2=w2.grad.reshape(b.K, b.H))
    out.update({"d" + k: v.grad for k, v in p.items()})
    out.update(st)
    return out


def _block_against_reference(name, got, deferred, tag):
    b, inp = lr.BLOCK[name], _inputs("block", name)
    _check_product(got["y1"], inp["w1"].double() @ inp["x"].double())
    want = lr.ref_block(inp, b.views, y1_forced=got["y1"].double(), y2_forced=got["y2"].double())
    if deferred:                                              # h is never written: the consumer normalised y1 on load
        assert torch.equal(got["h"], got["y1"])
        _check_product_on_load(got["y2"], inp["w2"].double() @ want["h"])
    else:
        _check_product(got["y2"], inp["w2"].double() @ got["h"].double())
    cmp = {k: v for k, v in got.items() if k != "h"}
    return _compare("block " + name, f"block {name} {tag}", cmp, want, b.M)


def _same_bits(a, b, keys=None):
    for k in keys or a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["tiny", "xl", "n64"])
def test_block_with_shortcut_token(name, monkeypatch):
    """The shortcut's gradient through the [W^T | I] product (one conv1x1_gemm_cat launch, S / XL / N64 tile) and through
    autograd's accumulation, against the same reference; prepared operands (ops.lowp_weights) and operands built on the
    fly give the same bits; the token is empty afterwards."""
    from grafp_amd import ops
    from grafp_amd._lib import lib
    b = lr.BLOCK[name]
    assert lr.plan_code(lib, b.K, b.H + b.K, 1, b.M, 1) == lr.CODE[b.cat]
    print(f"block {name}: concatenated data gradient {b.cat}, forward {b.fwd1} / {b.fwd2}, data gradient {b.dgrad2}")
    for fused in (True, False):
        monkeypatch.setattr(ops.switches, "shortcut_fusion", fused)
        counts = {}
        fly = _run_block(name, token=True, counts=counts)
        assert counts["token"] == fused and counts["cat"] == (1 if fused else 0) and counts["pro"] == 0, counts
        _block_against_reference(name, fly, False, "fused" if fused else "accumulate")
        prep = _run_block(name, token=True, prepared=True, counts=counts)
        assert counts["token"] == fused and counts["cat"] == (1 if fused else 0), counts
        _same_bits(fly, prep)


@pytest.mark.parametrize("token", [True, False], ids=["token", "no_token"])
@pytest.mark.parametrize("name", ["tiny-1v", "tiny", "n64", "n64-2v"])
def test_block_with_deferred_normalisation(name, token, monkeypatch):
    """The FFN form of stages 0 and 1: the producer (ReLU) leaves its (scale, shift) table, the consumer (<= 128 rows,
    residual) normalises on load in its product (n64: on the N64 tile) and in its weight gradient.  With
    switches.defer_norm off: the same z bits, gradients within the same bars."""
    from grafp_amd import ops
    from grafp_amd._lib import lib
    b = lr.BLOCK[name]
    assert lr.plan_code(lib, b.K, b.H, 1, b.M, b.views) == lr.CODE[b.fwd2]
    print(f"block {name}: deferred consumer on {b.fwd2}")
    assert ops.switches.defer_norm is True
    counts = {}
    got = _run_block(name, token=token, defer=True, counts=counts)
    assert counts["deferred"] and counts["pro"] == 1 and counts["token"] == token and counts["cat"] == int(token), counts
    _block_against_reference(name, got, True, "deferred" + (" + token" if token else ""))
    monkeypatch.setattr(ops.switches, "defer_norm", False)
    plain = _run_block(name, token=token, defer=True, counts=counts)
    assert not counts["deferred"] and counts["pro"] == 0, counts
    _same_bits(got, plain, ("z", "y1", "y2", "rm1", "rv1", "rm2", "rv2"))
    _block_against_reference(name, plain, False, "separate pass" + (" + token" if token else ""))


# ------------------------------------------------------------------------------------------------
# e. a derived, non-leaf weight (Downsample's tap matrix)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "xl"])
def test_layer_with_a_weight_derived_from_a_leaf(name):
    """w = a permuted slice of a parameter P (R, K/2, 2, 3): autograd scatters dW back through the views, so dW must be
    reduced when backward returns -- outside a defer_wgrad_reduce() block and inside one, where P.grad is read before
    the flush.  P.grad against the float64 dW, scattered the same way (zero outside the slice)."""
    from grafp_amd import ops
    c, inp = lr.CASE[name], _inputs("layer", name)
    half = c.K // 2
    got = _run_layer(name, lr.ACT_RELU)
    want = lr.ref_layer(inp, c.groups, c.views, lr.ACT_RELU, y_forced=got["y"].double())
    want_p = torch.zeros((c.R, half, 2, 3), dtype=torch.float64, device=DEV)
    want_p[:, :, :, 1] = want["dw"].reshape(c.R, 2, half).permute(0, 2, 1)

    def backward(deferred):
        P = torch.full((c.R, half, 2, 3), 0.25, device=DEV)
        P[:, :, :, 1] = inp["w"].reshape(c.R, 2, half).permute(0, 2, 1)
        P.requires_grad_(True)
        w = P[:, :, :, 1].permute(0, 2, 1).reshape(c.R, c.K)
        assert not w.is_leaf and torch.equal(w, inp["w"])
        x, gamma, beta, pb, res = (_leaf(inp[k]) for k in ("x", "gamma", "beta", "pb", "res"))
        z = ops.conv_bn_act(x, w, gamma, beta, inp["rm0"].clone(), inp["rv0"].clone(), True, lr.MOMENTUM, lr.EPS, pb, res,
                            lr.ACT_RELU, lr.SLOPE, c.groups, c.views)
        if deferred:
            with ops.defer_wgrad_reduce():
                z.backward(inp["dz"])
                assert len(ops._WGRAD_PENDING) == 0
                grad = P.grad.clone()                         # read before the flush at the end of the block
        else:
            z.backward(inp["dz"])
            grad = P.grad.clone()
        torch.cuda.synchronize()
        return grad

    plain, inside = backward(False), backward(True)
    assert torch.equal(plain, inside)
    assert torch.equal(plain[:, :, :, 1].permute(0, 2, 1).reshape(c.R, c.K), got["dw"])
    assert not bool(plain[:, :, :, 0].any()) and not bool(plain[:, :, :, 2].any())
    _compare(name, f"{name} derived weight", {"dw": plain.reshape(c.R, -1)}, {"dw": want_p.reshape(c.R, -1), "disputed": want["disputed"]},
             c.M)


# ------------------------------------------------------------------------------------------------
# the planted defects on the cases too large for the CPU suite (tests/test_layer_cpu.py runs the others)
# ------------------------------------------------------------------------------------------------
def test_planted_defects_exceed_the_bars_tenfold_on_the_large_cases():
    lr.assert_layer_defects_are_seen("n128", _inputs("layer", "n128"))
    lr.assert_block_defects_are_seen("n64-2v", _inputs("block", "n64-2v"))
