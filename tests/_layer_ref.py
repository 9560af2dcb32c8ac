"""Float64 autograd reference of the fused layer ops.conv_bn_act (grafp_amd/ops.py: _ConvBnAct) and of the two-layer
residual block built from it, with the table of cases tests/test_layer_cpu.py and tests/test_gpu_layer.py run (TEST
INFRASTRUCTURE).  Plain torch float64 with autograd: nothing here is imported from grafp_amd, no backward formula is
written out (test_layer_cpu.py pins it against nn.Conv2d + nn.BatchNorm2d).

One layer, on (rows, M) tensors whose M columns are `views` segments with statistics of their own:
    y = W x (group by group)                       stored in bf16
    u = (y + pre_bias - mean) * invstd * gamma + beta   mean, var over the ROUNDED y of a view (eval: running statistics)
    z = bf16(act(u) + residual)
A stored tensor is rounded by two casts (oracle.model.round_bf16), so the gradient passing through it is rounded to
bf16 where the HIP path stores it: dY behind the BatchNorm backward, dX behind the data-gradient product.

Forcing y: given `y_forced` (the bits the layer under test saved for its backward pass) the reference uses THOSE as the
value of y and still differentiates through W x.  Everything downstream is then float64 on identical y bits; without
it one rounding step of y next to a ReLU kink flips a mask element, which changes a whole column of dX.

Disputed elements: |u| <= 2^-20 (|y scale| + |shift|), the f32 resolution of the terms u is the sum of.  A kernel may
take the other side of the kink there; such an element's column leaves the per-element comparison of dX and its row
that of the row-wise gradients (DISPUTED_CAP bounds how many columns may go).

Planted defects (`defect=`): each restates one way the layer could be wrong, on the reference only; test_layer_cpu.py
asserts that every one of them exceeds the bars below by a factor of ten."""
import collections
import functools

import numpy as np
import torch

from _hashfill import hash_uniform

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.2
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
STEP = 2.0 ** -8                      # one bf16 rounding: the unit of the bf16 per-element metric
DISPUTED_CAP = 1e-3                   # at most 0.1 % of the columns of a case may hold a disputed element
SALT = "a/"                           # prefix of every hash name: chosen so that no small case holds a disputed element
TAIL = 128                            # the column tile of the S configuration: the last one of a view is what goes missing

# relative-L2 ceilings per tensor (tests/test_gpu_bf16_backward.py), literals
L2_ACT, L2_PARAM = 5e-3, 7e-3

CODE = {"S": 0, "L": 1, "N32": 2, "N64": 3, "N128": 4, "XL": 5}

# (K operand rows, R output rows, conv groups, M columns, views) and the tile configuration gemm_plan chooses for the
# forward product (R x K), the data gradient (K x R, one view) and the concatenated data gradient (K x (R + K))
Case = collections.namedtuple("Case", "name K R groups M views fwd dgrad cat")
CASES = [
    Case("tiny", 64, 64, 1, 256, 2, "S", "S", "S"),
    Case("large", 64, 512, 1, 512, 1, "L", "S", "S"),
    Case("xl", 512, 256, 1, 512, 2, "XL", "L", "XL"),
    Case("n32", 32, 32, 1, 65536, 1, "N32", "N32", "N32"),
    Case("n64", 64, 64, 1, 65536, 1, "N64", "N64", "N64"),
    Case("n128", 512, 128, 1, 131072, 1, "N128", "L", "XL"),
    Case("grouped", 128, 128, 4, 4096, 2, "S", "S", None),
    Case("views5", 64, 64, 1, 640, 5, "S", "S", "S"),
]
CASE = {c.name: c for c in CASES}
EVAL_CASES = ("tiny", "grouped", "xl")          # the cases that also run in eval mode

# x (K, M) -> layer 1 (K -> H, ReLU) -> layer 2 (H -> K, + x); fwd1 / fwd2: the two forward products, dgrad2: layer 2's
# data gradient, cat: layer 1's concatenated data gradient (K x (H + K)), dgrad1: the same without the shortcut rows
Block = collections.namedtuple("Block", "name K H M views fwd1 fwd2 dgrad2 cat dgrad1")
BLOCKS = [
    Block("tiny", 64, 256, 256, 2, "S", "S", "S", "S", "S"),
    Block("tiny-1v", 64, 256, 256, 1, "S", "S", "S", "S", "S"),
    Block("xl", 256, 1024, 512, 2, "L", "XL", "L", "XL", "XL"),
    Block("n64", 64, 256, 65536, 1, "S", "N64", "S", "N64", "N64"),
    Block("n64-2v", 64, 256, 131072, 2, "S", "N64", "S", "N64", "N64"),
]
BLOCK = {b.name: b for b in BLOCKS}

# Per-element bars per case and output = twice the worst deviation measured on the MI355X over every option of
# tests/test_gpu_layer.py that runs the case (the measured values: the table in that file's header); bf16 outputs in
# rounding steps, rounded up to whole steps, f32 outputs rounded up to two digits.  A zero bar: bit equality was measured
# (d residual is dz itself; d pre_bias under batch statistics is written as zero).
BARS = {
    "tiny": {"z": 1, "dx": 4, "dw": 0.00026, "dgamma": 3.2e-07, "dbeta": 1.8e-07, "dpb": 1.9e-07, "dres": 0, "rm": 4.8e-07, "rv": 2.2e-07},
    "large": {"z": 3, "dx": 4, "dw": 0.00019, "dgamma": 3.2e-07, "dbeta": 1.5e-07, "dpb": 0, "dres": 0, "rm": 2.5e-07, "rv": 3e-07},
    "xl": {"z": 3, "dx": 4, "dw": 7.7e-05, "dgamma": 2.6e-07, "dbeta": 1.8e-07, "dpb": 3.7e-07, "dres": 0, "rm": 9.5e-08, "rv": 1.6e-07},
    "n32": {"z": 4, "dx": 4, "dw": 0.00015, "dgamma": 7.8e-07, "dbeta": 2.1e-07, "dpb": 0, "dres": 0, "rm": 2.3e-07, "rv": 1.6e-07},
    "n64": {"z": 4, "dx": 4, "dw": 7.8e-05, "dgamma": 4.6e-07, "dbeta": 1.8e-07, "dpb": 0, "dres": 0, "rm": 3.7e-07, "rv": 2e-07},
    "n128": {"z": 4, "dx": 4, "dw": 6.7e-05, "dgamma": 3.9e-07, "dbeta": 2.9e-07, "dpb": 0, "dres": 0, "rm": 3e-07, "rv": 1.6e-07},
    "grouped": {"z": 4, "dx": 5, "dw": 0.0005, "dgamma": 9.2e-07, "dbeta": 2.1e-07, "dpb": 2.2e-07, "dres": 0, "rm": 1.3e-07, "rv": 3.9e-07},
    "views5": {"z": 1, "dx": 3, "dw": 0.00028, "dgamma": 2.7e-07, "dbeta": 2.9e-07, "dpb": 0, "dres": 0, "rm": 1.5e-07, "rv": 3.6e-07},
    "block tiny": {"z": 0, "dx": 4, "dw1": 6.6e-05, "dw2": 2.1e-07, "dgamma1": 7.8e-05, "dgamma2": 2.3e-07,
                   "dbeta1": 5.1e-05, "dbeta2": 3.7e-08, "dpb1": 0, "dpb2": 0, "rm1": 3.1e-07, "rv1": 2.6e-07,
                   "rm2": 2.7e-07, "rv2": 2.1e-07},
    "block xl": {"z": 2, "dx": 4, "dw1": 0.0011, "dw2": 0.00091, "dgamma1": 0.0008, "dgamma2": 2e-07,
                 "dbeta1": 0.00095, "dbeta2": 4.6e-08, "dpb1": 0, "dpb2": 0, "rm1": 2.3e-07, "rv1": 1.3e-07,
                 "rm2": 2.6e-07, "rv2": 2.4e-07},
    "block n64": {"z": 4, "dx": 6, "dw1": 0.00014, "dw2": 8.7e-05, "dgamma1": 0.00013, "dgamma2": 2.5e-07,
                  "dbeta1": 0.00011, "dbeta2": 4.4e-07, "dpb1": 0, "dpb2": 0, "rm1": 2.8e-07, "rv1": 1.8e-07,
                  "rm2": 1.5e-07, "rv2": 1.5e-07},
    "block tiny-1v": {"z": 0, "dx": 4, "dw1": 9.5e-06, "dw2": 2.7e-07, "dgamma1": 2.4e-07, "dgamma2": 2.8e-07,
                      "dbeta1": 2.1e-08, "dbeta2": 3.8e-08, "dpb1": 0, "dpb2": 0, "rm1": 1.8e-07, "rv1": 1.8e-07,
                      "rm2": 2.5e-07, "rv2": 1.4e-07},
    "block n64-2v": {"z": 4, "dx": 6, "dw1": 0.00013, "dw2": 0.00016, "dgamma1": 0.00012, "dgamma2": 3.7e-07,
                     "dbeta1": 0.00014, "dbeta2": 1.9e-07, "dpb1": 0, "dpb2": 0, "rm1": 3.5e-07, "rv1": 3.2e-07,
                     "rm2": 2e-07, "rv2": 3.3e-07},
}
BF16_OUT = ("z", "dx", "dres")


def plan_code(lib, R, K, groups, M, views):
    """Tile configuration of the R x K product over M columns (grafp_conv1x1_gemm_plan, a host function)."""
    import ctypes
    info = (ctypes.c_int * 8)()
    assert lib.grafp_conv1x1_gemm_plan(R, K, groups, M, views, info) == 0, (R, K, groups, M, views)
    return info[0]


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def _operand(name, rows, M, views):
    """bf16 (rows, M): unit-variance noise, view v scaled by 1 + v/2 and shifted by v; where a view is longer than TAIL
    its last TAIL columns are shifted by 4 more, so that leaving them out is seen by a sum over the view."""
    Mg = M // views
    a = hash_uniform(name, (rows, views, Mg)) * np.float32(np.sqrt(3.0))
    v = np.arange(views, dtype=np.float32)[None, :, None]
    a = a * (1.0 + 0.5 * v) + v
    if Mg > TAIL:
        a[:, :, Mg - TAIL:] += 4.0
    return _bf16(a.reshape(rows, M))


def _noise(name, rows, M):
    return _bf16(hash_uniform(name, (rows, M)) * np.float32(np.sqrt(3.0)))


def _weight(name, R, Kg):
    """(R, Kg) f32 holding bf16 values, variance 1 / Kg: the layer's bf16 copy is the weight itself."""
    return _bf16(hash_uniform(name, (R, Kg)) * np.float32(np.sqrt(3.0 / Kg))).float()


def _rows(R, tag):
    """gamma, beta, pre_bias, running mean, running variance: distinct ramps per row."""
    r = torch.arange(R, dtype=torch.float32) / max(R - 1, 1)
    return {"gamma" + tag: 0.5 + r, "beta" + tag: 0.4 * r - 0.2, "pb" + tag: 1.0 - 2.0 * r,
            "rm0" + tag: 0.6 * r - 0.3, "rv0" + tag: 0.5 + 1.5 * r.flip(0)}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """The tensors of a CASES row (CPU): x (K, M), res / dz (R, M) in bf16, everything else f32."""
    c = CASE[name]
    d = {"x": _operand(f"{SALT}layer:{name}:x", c.K, c.M, c.views), "w": _weight(f"{SALT}layer:{name}:w", c.R, c.K // c.groups),
         "res": _noise(f"{SALT}layer:{name}:res", c.R, c.M), "dz": _noise(f"{SALT}layer:{name}:dz", c.R, c.M)}
    d.update(_rows(c.R, ""))
    return d


@functools.lru_cache(maxsize=None)
def block_inputs(name):
    """The tensors of a BLOCKS row: x, dz (K, M) bf16; w1 (H, K), w2 (K, H); the row parameters of both layers."""
    b = BLOCK[name]
    d = {"x": _operand(f"{SALT}block:{name}:x", b.K, b.M, b.views), "dz": _noise(f"{SALT}block:{name}:dz", b.K, b.M),
         "w1": _weight(f"{SALT}block:{name}:w1", b.H, b.K), "w2": _weight(f"{SALT}block:{name}:w2", b.K, b.H)}
    d.update(_rows(b.H, "1"))
    d.update(_rows(b.K, "2"))
    return d


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def round_bf16(t):
    """oracle.model.round_bf16 on float64: rounds the value, and under autograd the gradient passing through."""
    return t.to(torch.bfloat16).to(t.dtype)


class _Force(torch.autograd.Function):
    """The value of `forced`, the derivative of the identity: y keeps its place in the graph and takes the given bits."""

    @staticmethod
    def forward(ctx, y, forced):
        return forced.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _product(w, x, groups):
    R, Kg = w.shape
    M = x.shape[1]
    return torch.bmm(w.reshape(groups, R // groups, Kg), x.reshape(groups, Kg, M)).reshape(R, M)


def _layer(x, w, gamma, beta, pb, res, rm0, rv0, groups, views, act, slope, training, y_forced, rounding, defect):
    """-> z and what the drivers read: the product node (its .grad is the stored dY), the rounded y, the running
    statistics after the pass, the disputed mask (R, M)."""
    q = round_bf16 if rounding else (lambda t: t)
    R, M = w.shape[0], x.shape[1]
    yp = _product(w, x, groups)
    yp.retain_grad()
    y = q(yp if y_forced is None else _Force.apply(yp, y_forced))
    sv = 1 if defect == "batch_statistics" else views
    yv = y.reshape(R, sv, M // sv)
    b = torch.zeros_like(gamma) if pb is None else pb
    rm, rv = rm0, rv0
    if training:
        src = yv[:, :, :-TAIL] if defect == "statistics_tail" else yv
        n = src.shape[2]
        mean, var = src.mean(dim=2) + b[:, None], src.var(dim=2, unbiased=False)
        for v in range(sv):                                    # once per view, in view order, unbiased variance
            rm = (1.0 - MOMENTUM) * rm + MOMENTUM * mean[:, v].detach()
            rv = (1.0 - MOMENTUM) * rv + MOMENTUM * var[:, v].detach() * (n / (n - 1.0))
        if defect == "views_swapped":
            mean, var = mean.roll(1, dims=1), var.roll(1, dims=1)
    else:
        mean, var = rm0[:, None].expand(R, sv), rv0[:, None].expand(R, sv)
    invstd = torch.rsqrt(var + EPS)
    u = (yv + b[:, None, None] - mean[:, :, None]) * invstd[:, :, None] * gamma[:, None, None] + beta[:, None, None]
    with torch.no_grad():
        scale = gamma[:, None] * invstd
        shift = beta[:, None] + (b[:, None] - mean) * scale
        disputed = (u.abs() <= 2.0 ** -20 * ((yv * scale[:, :, None]).abs() + shift.abs()[:, :, None])).reshape(R, M)
        if act == ACT_NONE:
            disputed = torch.zeros_like(disputed)              # no kink to be on the other side of
    u = u.reshape(R, M)
    if act == ACT_RELU:
        a = torch.relu(u)
    elif act == ACT_LEAKY:
        a = torch.where(u > 0, u, slope * u)
        if defect == "slope_ignored":                          # the forward value, ReLU's derivative
            a = torch.relu(u) + (slope * torch.clamp(u, max=0.0)).detach()
    else:
        a = u
    z = q(a if res is None else a + res)
    return z, dict(yp=yp, y=y.detach(), rm=rm, rv=rv, disputed=disputed)


def _leaf(t, dev=None):
    return t.detach().to(device=dev, dtype=torch.float64).clone().requires_grad_(True)


def _tail_mask(M, views, like):
    keep = torch.ones((views, M // views), dtype=like.dtype, device=like.device)
    keep[:, -TAIL:] = 0
    return keep.reshape(1, M)


def ref_layer(inp, groups, views, act, training=True, use_pb=True, use_res=True, y_forced=None, rounding=True,
              defect=None, slope=SLOPE):
    """Forward + backward of one layer on the tensors of `inp` (on their device) -> float64 results:
    z, y, dx, dw, dgamma, dbeta, dpb (None without pre_bias; 0 under batch statistics), dres, rm, rv, disputed."""
    q = round_bf16 if rounding else (lambda t: t)
    x, w, gamma, beta = _leaf(inp["x"]), _leaf(inp["w"]), _leaf(inp["gamma"]), _leaf(inp["beta"])
    pb = _leaf(inp["pb"]) if use_pb else None
    res = _leaf(inp["res"]) if use_res else None
    z, aux = _layer(q(x), w, gamma, beta, pb, None if res is None else q(res), inp["rm0"].double(), inp["rv0"].double(),
                    groups, views, act, slope, training, y_forced, rounding, defect)
    z.backward(inp["dz"].double())
    dy = aux["yp"].grad
    out = dict(z=z.detach(), y=aux["y"], dx=x.grad, dw=w.grad, dgamma=gamma.grad, dbeta=beta.grad,
               dpb=None if pb is None else (torch.zeros_like(pb.grad) if training else pb.grad),
               dres=None if res is None else res.grad, rm=aux["rm"], rv=aux["rv"], disputed=aux["disputed"])
    xd, wd = x.detach(), w.detach()
    if defect == "dpb_zero":
        out["dpb"] = torch.zeros_like(out["dpb"])
    elif defect == "group_transpose":                          # the ungrouped transpose read as the grouped operand
        R, Kg = wd.shape
        out["dx"] = q(_product(wd.t().contiguous().reshape(groups * Kg, R // groups), dy, groups))
    elif defect == "dw_tail":
        out["dw"] = _dw(dy * _tail_mask(xd.shape[1], views, dy), xd, groups)
    return out


def _dw(dy, x, groups):
    R, M = dy.shape
    K = x.shape[0]
    return torch.bmm(dy.reshape(groups, R // groups, M), x.reshape(groups, K // groups, M).transpose(1, 2)).reshape(R, K // groups)


def ref_block(inp, views, y1_forced=None, y2_forced=None, rounding=True, defect=None):
    """x -> layer 1 (ReLU) -> h -> layer 2 (+ x), both with pre_bias, in training mode -> float64 results: z, y1, y2,
    h, dx, dw1, dw2, dgamma1/2, dbeta1/2, dpb1/2, rm1/2, rv1/2, disputed (of layer 1, (H, M)).  The deferred form of the
    layer under test hands its consumer the raw y1 and layer 1's (scale, shift, ReLU): h is the same tensor."""
    q = round_bf16 if rounding else (lambda t: t)
    x = _leaf(inp["x"])
    p = {k: _leaf(inp[k]) for k in ("w1", "w2", "gamma1", "gamma2", "beta1", "beta2", "pb1", "pb2")}
    xin = q(x)
    d1 = defect if defect in ("batch_statistics", "views_swapped", "statistics_tail") else None
    h, a1 = _layer(xin, p["w1"], p["gamma1"], p["beta1"], p["pb1"], None, inp["rm01"].double(), inp["rv01"].double(), 1,
                   views, ACT_RELU, 0.0, True, y1_forced, rounding, d1)
    short = xin
    if defect == "shortcut_dropped":
        short = xin.detach()
    elif defect == "shortcut_doubled":
        short = 2.0 * xin - xin.detach()
    elif defect == "identity_rows":
        short = xin.detach()                                   # added below, on the wrong rows
    z, a2 = _layer(h, p["w2"], p["gamma2"], p["beta2"], p["pb2"], short, inp["rm02"].double(), inp["rv02"].double(), 1,
                   views, ACT_NONE, 0.0, True, y2_forced, rounding, None)
    dz = inp["dz"].double()
    z.backward(dz)
    out = dict(z=z.detach(), y1=a1["y"], y2=a2["y"], h=h.detach(), dx=x.grad, dw1=p["w1"].grad, dw2=p["w2"].grad,
               dgamma1=p["gamma1"].grad, dgamma2=p["gamma2"].grad, dbeta1=p["beta1"].grad, dbeta2=p["beta2"].grad,
               dpb1=torch.zeros_like(p["pb1"].grad), dpb2=torch.zeros_like(p["pb2"].grad),
               rm1=a1["rm"], rv1=a1["rv"], rm2=a2["rm"], rv2=a2["rv"], disputed=a1["disputed"])
    if defect == "identity_rows":                              # [W^T | I] with the identity one row block down
        out["dx"] = q(p["w1"].detach().t() @ a1["yp"].grad + dz.roll(32, dims=0))
    elif defect == "dw_raw_operand":                           # the consumer's dW on the producer's raw output
        out["dw2"] = a2["yp"].grad @ a1["y"].t()
    elif defect == "dw_tail":
        out["dw2"] = (a2["yp"].grad * _tail_mask(dz.shape[1], views, dz)) @ h.detach().t()
    return out


# ------------------------------------------------------------------------------------------------
# metrics
# ------------------------------------------------------------------------------------------------
def err_bf16(got, want):
    """Per element, in rounding steps: |got - want| / (2^-8 max(|want|, row RMS of want))."""
    got, want = got.double(), want.double()
    rms = want.pow(2).mean(dim=1, keepdim=True).sqrt()
    return (got - want).abs() / (STEP * torch.maximum(want.abs(), rms))


def err_f32(got, want):
    """Per element: |got - want| / max |want|."""
    got, want = got.double(), want.double()
    return (got - want).abs() / want.abs().max()


def rel_l2(got, want):
    got, want = got.double(), want.double()
    return float((got - want).norm() / want.norm())


def base_name(key):
    """dw2 -> dw, rm1 -> rm: the bar of a block's output is the bar of the layer's."""
    return key.rstrip("12")


def worst(got, want, disputed=None, keys=None):
    """{output: (worst per-element metric outside the disputed positions, relative L2 over everything)} for the outputs
    both sides have.  disputed (rows, M) of the layer whose columns feed dx: its columns leave dx; per layer the rows
    leave dw, dgamma, dbeta, dpb (the block's mask belongs to layer 1)."""
    res = {}
    cols = rows = None
    if disputed is not None and bool(disputed.any()):
        cols, rows = disputed.any(dim=0), disputed.any(dim=1)
    for k in keys or [k for k in got if k in want and k in OUTPUTS and got[k] is not None and want[k] is not None]:
        g, w = got[k].double().reshape(want[k].shape), want[k].double()
        b = base_name(k)
        if b == "dpb" and not bool(w.any()):                   # batch statistics: exactly zero on both sides
            res[k] = (0.0 if not bool(g.any()) else float("inf"), 0.0)
            continue
        e = err_bf16(g, w) if b in BF16_OUT else err_f32(g.reshape(w.shape[0], -1), w.reshape(w.shape[0], -1))
        if cols is not None and b == "dx":
            e = e[:, ~cols]
        elif rows is not None and b in ("dw", "dgamma", "dbeta", "dpb") and not k.endswith("2"):
            e = e[~rows]
        res[k] = (float(e.max()) if e.numel() else 0.0, rel_l2(g, w))
    return res


OUTPUTS = {b + s for b in ("z", "dx", "dres", "dw", "dgamma", "dbeta", "dpb", "rm", "rv") for s in ("", "1", "2")}


# ------------------------------------------------------------------------------------------------
# sharpness: the planted defects, where each applies, and how far beyond the bars it lands
# ------------------------------------------------------------------------------------------------
DEFECTS = {"shortcut_dropped", "shortcut_doubled", "group_transpose", "batch_statistics", "views_swapped", "dpb_zero",
           "slope_ignored", "dw_raw_operand", "identity_rows", "dw_tail", "statistics_tail"}


def layer_defects(c):
    """(defect, activation, training) that apply to a CASES row (eval mode: the cases that run it)."""
    out = [("slope_ignored", ACT_LEAKY, True)]
    if c.name in EVAL_CASES:
        out.append(("dpb_zero", ACT_RELU, False))
    if c.groups > 1:
        out.append(("group_transpose", ACT_RELU, True))
    if c.views > 1:
        out += [("batch_statistics", ACT_RELU, True), ("views_swapped", ACT_RELU, True)]
    if c.M // c.views > TAIL:
        out += [("dw_tail", ACT_RELU, True), ("statistics_tail", ACT_RELU, True)]
    return out


def block_defects(b):
    out = ["shortcut_dropped", "shortcut_doubled", "identity_rows", "dw_raw_operand"]
    if b.views > 1:
        out += ["batch_statistics", "views_swapped"]
    if b.M // b.views > TAIL:
        out += ["dw_tail", "statistics_tail"]
    return out


def excess(bad, good, bars):
    """Largest (per-element deviation / bar) over the outputs, the disputed positions of the good side left out."""
    w = worst(bad, good, good["disputed"])
    return max(((v[0] / bars[k] if bars[k] > 0 else (float("inf") if v[0] > 0 else 0.0)), k) for k, v in w.items())


def assert_layer_defects_are_seen(name, inp):
    """Every defect that applies to the case, planted in the reference, against the reference: >= 10 bars."""
    c = CASE[name]
    good = {}
    for defect, act, training in layer_defects(c):
        if (act, training) not in good:
            good[act, training] = ref_layer(inp, c.groups, c.views, act, training)
        ratio, key = excess(ref_layer(inp, c.groups, c.views, act, training, defect=defect), good[act, training], BARS[name])
        print(f"{name}: {defect}: {ratio:.1f} bars on {key}")
        assert ratio >= 10.0, (name, defect, ratio, key)


def assert_block_defects_are_seen(name, inp):
    b = BLOCK[name]
    good = ref_block(inp, b.views)
    for defect in block_defects(b):
        ratio, key = excess(ref_block(inp, b.views, defect=defect), good, BARS["block " + name])
        print(f"block {name}: {defect}: {ratio:.1f} bars on {key}")
        assert ratio >= 10.0, (name, defect, ratio, key)
