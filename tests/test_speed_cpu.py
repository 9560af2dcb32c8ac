"""Speed augmentation without a GPU: the float64 rule of csrc/speed.hip against the polyphase resampler's restatement,
the two host helpers that size the input, the cfg keys, and the build flags of speed.hip."""
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _corpus_ref import resample_f64
from _speed_ref import speed_f32, speed_f64, tap_range, uniform_rows
from grafp_amd import ops
from grafp_amd.modules.transformations import GPUTransformNeuralfp
from grafp_amd.util import load_config

PAIRS = ((26, 25), (25, 26), (128, 123), (2, 1), (1, 2), (1, 1))


@pytest.mark.parametrize("orig,new", PAIRS)
def test_rule_in_f64_is_the_polyphase_resampler_at_rational_ratios(orig, new):
    """speed_f64 at rho = orig / new, x_offset = 0, equals _corpus_ref.resample_f64 (measured: 1e-12 at most).  At 1/1 the
    filter is evaluated (copy_at_one=False): the resampler's restatement has no copy branch."""
    x = uniform_rows(1, 3000, 11)[0]
    want = resample_f64(x, orig, new)
    got = speed_f64(x, orig / new, want.size, 0, copy_at_one=False)
    err = np.abs(got - want).max()
    print(f"{orig}/{new}: {err:.2e}")
    assert err <= 1e-11


def test_the_f32_route_stays_near_the_rule():
    """e32, the error bar's unit of tests/test_gpu_speed.py: a few 1e-7 on uniform [-1, 1] input."""
    x = uniform_rows(1, 2500, 12)[0]
    for rho in (0.5, 0.94, np.nextafter(np.float32(1), np.float32(2)), 1.06, 2.0):
        r = np.float32(rho)
        e32 = np.abs(speed_f32(x, r, 1000, 14) - speed_f64(x, float(r), 1000, 14)).max()
        print(f"rho={rho}: e32 = {e32:.2e}")
        assert 0 < e32 < 1e-6
    assert np.array_equal(speed_f32(x, 1.0, 1000, 3), x[3:1003])


@pytest.mark.parametrize("ratio", (0.5, 0.94, 1.0, 1.06, 2.0))
@pytest.mark.parametrize("out_len", (1, 2, 700, 16000))
def test_speed_input_len_keeps_every_tap_inside(ratio, out_len):
    """With x_offset = speed_pad(r) and T_in = speed_input_len(out_len, r), brute force over the rule's tap ranges of every
    output, at r and at ratios below it: no tap outside [0, T_in).  The formulas round the filter's reach up and add one,
    so the spare room is small but not zero: the outermost taps lie within three samples of either end (an input one
    sample shorter would still hold every tap of the rule; what it would no longer hold is the kernel's staged window)."""
    pad, T_in = ops.speed_pad(ratio), ops.speed_input_len(out_len, ratio)
    reach = 6.0 / (0.99 * min(1.0, 1.0 / ratio))
    assert pad == int(np.ceil(reach)) + 1
    assert T_in == pad + int(np.ceil((out_len - 1) * ratio)) + 1 + pad
    m = np.arange(out_len, dtype=np.float64)
    for rho in sorted({ratio, max(0.5, ratio * 0.97), 0.5}):
        klo, khi = tap_range(pad + m * rho, rho)
        assert klo.min() >= 0 and khi.max() < T_in, (rho, klo.min(), khi.max(), T_in)
    klo, khi = tap_range(pad + m * ratio, ratio)
    assert klo.min() <= 2 and khi.max() >= T_in - 4, (klo.min(), khi.max(), T_in)
    # the candidates the kernel stages, floor(p) - W .. floor(p) + W + 1 with W = floor(reach), are inside too
    fl = np.floor(pad + m * ratio).astype(np.int64)
    assert fl.min() - int(reach) >= 0 and fl.max() + int(reach) + 1 < T_in


def test_speed_input_len_at_the_training_shape():
    assert ops.speed_pad(1.06) == 8 and ops.speed_input_len(16000, 1.06) == 16976
    assert ops.speed_pad(1.0) == 8 and ops.speed_pad(0.5) == 8 and ops.speed_pad(2.0) == 14


def _cfg(**kw):
    return dict(load_config(), **kw)


@pytest.mark.parametrize("bad", ([0.4, 1.0], [1.0, 2.1], [1.1, 1.0], [1.0], "fast", [float("nan"), 1.0]))
def test_bad_speed_ranges_are_refused(bad):
    with pytest.raises(ValueError, match="speed_range"):
        GPUTransformNeuralfp(_cfg(speed_prob=0.5, speed_range=bad), None, None, train=True)
    with pytest.raises(ValueError, match="speed_range"):        # also while the augmentation is off
        ops.speed_config(_cfg(speed_range=bad))


def test_speed_prob_needs_a_range_and_is_a_probability():
    with pytest.raises(ValueError, match="speed_range"):
        GPUTransformNeuralfp(_cfg(speed_prob=0.5), None, None, train=True)
    with pytest.raises(ValueError, match="speed_prob"):
        GPUTransformNeuralfp(_cfg(speed_prob=1.5, speed_range=[0.9, 1.1]), None, None, train=True)
    for off in ({}, {"speed_prob": 0}, {"speed_prob": 0.0, "speed_range": [0.94, 1.06]}, {"speed_range": [0.94, 1.06]}):
        t = GPUTransformNeuralfp(_cfg(**off), None, None, train=True)
        assert t.speed is None and t.pad == 0 and t.draw_len == 16000
    t = GPUTransformNeuralfp(_cfg(speed_prob=0.5, speed_range=[0.94, 1.06]), None, None, train=True)
    assert t.speed == (0.5, 0.94, 1.06) and t.pad == 8 and t.draw_len == 16976 and t.clip == 16000


def test_shipped_config_has_no_speed_keys():
    cfg = load_config()
    assert "speed_prob" not in cfg and "speed_range" not in cfg


@pytest.mark.parametrize("shape_i,shape_j", (((4, 16000), (4, 16000)), ((4, 16976), (4, 16000)), ((4, 16975), (4, 16975)),
                                             ((16976,), (16976,))))
def test_forward_refuses_a_wrong_view_length_and_names_draw_len(shape_i, shape_j):
    t = GPUTransformNeuralfp(_cfg(speed_prob=1.0, speed_range=[0.94, 1.06]), None, None, train=True)
    with pytest.raises(ValueError, match=r"draw_len = 16976"):
        t(torch.zeros(shape_i), torch.zeros(shape_j))


def test_speed_change_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.speed_change(torch.zeros(2, 100), torch.ones(2), 50)


def test_entry_reports_argument_errors_without_a_gpu():
    from grafp_amd._lib import lib
    one = 1 << 12                                            # any non-null address: the checks come before the launch
    assert lib.grafp_speed_change_f32(None, 10, 1, 10, 0, one, one, 10, 10, None) == -1
    assert b"null pointer" in lib.grafp_last_error()
    for args, what in (((one, 10, 0, 10, 0, one, one * 2, 10, 10, None), b"bad sizes"),
                       ((one, 9, 1, 10, 0, one, one * 2, 10, 10, None), b"row strides"),
                       ((one, 10, 1, 10, 0, one, one * 2, 9, 10, None), b"row strides"),
                       ((one, 10, 1, 10, 0, one, one, 10, 10, None), b"alias"),
                       ((one, 10, 1, 10, -1, one, one * 2, 10, 10, None), b"x_offset"),
                       # two faults at once: the checks shared with time_stretch (csrc/clipwarp.h) keep their order
                       ((one, 10, 1, 10, -1, one, one, 10, 10, None), b"alias")):
        assert lib.grafp_speed_change_f32(*args) == -1 and what in lib.grafp_last_error(), what


def test_speed_kernel_has_no_packed_high_register_select():
    """The shipped object's own command (make -n), compiled to device assembly: no packed-f32 instruction at all in
    speed.hip, and the tap sum is an fma chain."""
    asm = shipped_asm("speed")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert any("speed_change_kernel" in k for k in kernels)
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm
