"""CPU tests of the layer reference (tests/_layer_ref.py) that tests/test_gpu_layer.py compares ops.conv_bn_act with:
it equals torch's own Conv2d + BatchNorm2d autograd when nothing is rounded, its case table reaches the tile
configurations it names, its disputed elements are rare, and every planted defect exceeds the bars by a factor of ten."""
import pytest
import torch
import torch.nn.functional as F

import _layer_ref as lr

SMALL = ["tiny", "large", "xl", "grouped", "views5"]          # the cases up to M = 4096
ON_CPU = SMALL + ["n32", "n64"]                               # n128 and the block n64-2v: tests/test_gpu_layer.py
BLOCKS_ON_CPU = ["tiny", "tiny-1v", "xl", "n64"]


# ------------------------------------------------------------------------------------------------
# the reference is independent: nn.Conv2d + nn.BatchNorm2d + activation, float64 autograd, nothing rounded
# ------------------------------------------------------------------------------------------------
def _nn_layer(x, w, gamma, beta, pb, rm0, rv0, groups, views, act, training):
    """(K, M) -> (R, M) through torch's modules, a view at a time (columns = the batch): -> act(bn(conv(x))), conv, bn."""
    R, Kg = w.shape
    conv = torch.nn.Conv2d(Kg * groups, R, 1, groups=groups, bias=pb is not None).double()
    bn = torch.nn.BatchNorm2d(R, eps=lr.EPS, momentum=lr.MOMENTUM).double()
    with torch.no_grad():
        conv.weight.copy_(w.reshape(R, Kg, 1, 1))
        if pb is not None:
            conv.bias.copy_(pb)
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    bn.train(training)
    u = torch.cat([bn(conv(xv.t().reshape(xv.shape[1], -1, 1, 1))).reshape(xv.shape[1], R).t()
                   for xv in x.chunk(views, dim=1)], dim=1)
    a = torch.relu(u) if act == lr.ACT_RELU else (F.leaky_relu(u, lr.SLOPE) if act == lr.ACT_LEAKY else u)
    return a, conv, bn


def _close(got, want, what):
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= 1e-12 * scale, (what, err, scale)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("act", [lr.ACT_NONE, lr.ACT_RELU, lr.ACT_LEAKY])
@pytest.mark.parametrize("name", ["tiny", "grouped", "views5"])
def test_reference_layer_equals_torch_modules_when_nothing_is_rounded(name, act, training):
    c, inp = lr.CASE[name], lr.case_inputs(name)
    for use_pb, use_res in ((True, True), (True, False), (False, True), (False, False)):
        got = lr.ref_layer(inp, c.groups, c.views, act, training, use_pb, use_res, rounding=False)
        x = lr._leaf(inp["x"])
        res = lr._leaf(inp["res"]) if use_res else None
        a, conv, bn = _nn_layer(x, inp["w"].double(), inp["gamma"].double(), inp["beta"].double(),
                                inp["pb"].double() if use_pb else None, inp["rm0"].double(), inp["rv0"].double(), c.groups,
                                c.views, act, training)
        z = a + res if use_res else a
        z.backward(inp["dz"].double())
        what = (name, act, training, use_pb, use_res)
        _close(got["z"], z.detach(), what + ("z",))
        _close(got["dx"], x.grad, what + ("dx",))
        _close(got["dw"], conv.weight.grad.reshape(got["dw"].shape), what + ("dw",))
        _close(got["dgamma"], bn.weight.grad, what + ("dgamma",))
        _close(got["dbeta"], bn.bias.grad, what + ("dbeta",))
        _close(got["rm"], bn.running_mean, what + ("rm",))
        _close(got["rv"], bn.running_var, what + ("rv",))
        if use_pb:
            _close(got["dpb"], conv.bias.grad, what + ("dpb",))       # under batch statistics: rounding noise against exact zero
        if use_res:
            _close(got["dres"], res.grad, what + ("dres",))


@pytest.mark.parametrize("name", ["tiny", "tiny-1v"])
def test_reference_block_equals_torch_modules_when_nothing_is_rounded(name):
    """The block of the shortcut and the deferred-normalisation tests: one reference for both (the deferred form is the
    same function of x)."""
    b, inp = lr.BLOCK[name], lr.block_inputs(name)
    got = lr.ref_block(inp, b.views, rounding=False)
    x = lr._leaf(inp["x"])
    d = {k: v.double() for k, v in inp.items()}
    h, conv1, bn1 = _nn_layer(x, d["w1"], d["gamma1"], d["beta1"], d["pb1"], d["rm01"], d["rv01"], 1, b.views, lr.ACT_RELU, True)
    a, conv2, bn2 = _nn_layer(h, d["w2"], d["gamma2"], d["beta2"], d["pb2"], d["rm02"], d["rv02"], 1, b.views, lr.ACT_NONE, True)
    z = a + x
    z.backward(inp["dz"].double())
    _close(got["z"], z.detach(), "z")
    _close(got["h"], h.detach(), "h")
    _close(got["dx"], x.grad, "dx")
    for i, conv, bn in (("1", conv1, bn1), ("2", conv2, bn2)):
        _close(got["dw" + i], conv.weight.grad.reshape(got["dw" + i].shape), "dw" + i)
        _close(got["dgamma" + i], bn.weight.grad, "dgamma" + i)
        _close(got["dbeta" + i], bn.bias.grad, "dbeta" + i)
        _close(got["rm" + i], bn.running_mean, "rm" + i)
        _close(got["rv" + i], bn.running_var, "rv" + i)


# ------------------------------------------------------------------------------------------------
# the case table holds
# ------------------------------------------------------------------------------------------------
def test_every_case_reaches_the_tile_configurations_its_row_names():
    from grafp_amd import ops
    from grafp_amd._lib import lib
    for c in lr.CASES:
        assert ops.gemm_supported(c.R, c.K, c.groups, c.M, c.views) and ops.gemm_supported(c.K, c.R, c.groups, c.M, 1), c
        assert lr.plan_code(lib, c.R, c.K, c.groups, c.M, c.views) == lr.CODE[c.fwd], c
        assert lr.plan_code(lib, c.K, c.R, c.groups, c.M, 1) == lr.CODE[c.dgrad], c
        if c.cat is not None:
            assert ops.gemm_supported(c.K, c.R + c.K, 1, c.M, 1), c
            assert lr.plan_code(lib, c.K, c.R + c.K, 1, c.M, 1) == lr.CODE[c.cat], c
    for b in lr.BLOCKS:
        for R, K, views, want in ((b.H, b.K, b.views, b.fwd1), (b.K, b.H, b.views, b.fwd2), (b.H, b.K, 1, b.dgrad2),
                                  (b.K, b.H + b.K, 1, b.cat), (b.K, b.H, 1, b.dgrad1)):
            assert ops.gemm_supported(R, K, 1, b.M, views), (b, R, K)
            assert lr.plan_code(lib, R, K, 1, b.M, views) == lr.CODE[want], (b, R, K, want)
    # every forward configuration; L and an N tile for the data gradient; S, XL and an N tile for the concatenated product
    assert {c.fwd for c in lr.CASES} == set(lr.CODE)
    assert {"L", "N32", "N64"} <= {c.dgrad for c in lr.CASES}
    assert {"S", "XL", "N64"} <= {b.cat for b in lr.BLOCKS}
    assert lr.BLOCK["n64"].fwd2 == lr.BLOCK["n64-2v"].fwd2 == "N64"          # a deferred consumer on an N tile


# ------------------------------------------------------------------------------------------------
# disputed elements are rare
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_disputed_elements_stay_under_the_cap(name):
    c, inp = lr.CASE[name], lr.case_inputs(name)
    for act in (lr.ACT_RELU, lr.ACT_LEAKY):
        for training in (True, False):
            d = lr.ref_layer(inp, c.groups, c.views, act, training)["disputed"]
            assert float(d.any(dim=0).double().mean()) <= lr.DISPUTED_CAP, (name, act, training, int(d.sum()))
            assert float(d.double().mean()) <= 1e-4, (name, act, training, int(d.sum()))      # about 1e-6 expected
    assert not bool(lr.ref_layer(inp, c.groups, c.views, lr.ACT_NONE)["disputed"].any())


# ------------------------------------------------------------------------------------------------
# sharpness: every planted defect exceeds the bars by a factor of ten wherever it applies
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ON_CPU)
def test_planted_layer_defects_exceed_the_bars_tenfold(name):
    lr.assert_layer_defects_are_seen(name, lr.case_inputs(name))


@pytest.mark.parametrize("name", BLOCKS_ON_CPU)
def test_planted_block_defects_exceed_the_bars_tenfold(name):
    lr.assert_block_defects_are_seen(name, lr.block_inputs(name))


def test_every_listed_defect_is_planted_somewhere():
    seen = {d for c in lr.CASES for d, _, _ in lr.layer_defects(c)} | {d for b in lr.BLOCKS for d in lr.block_defects(b)}
    assert seen == lr.DEFECTS
