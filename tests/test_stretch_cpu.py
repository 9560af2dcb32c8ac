"""Time-stretch augmentation without a GPU: the invariants of the float64 rule of csrc/stretch.hip (tests/_stretch_ref.py),
the condition on the inputs of tests/test_gpu_stretch.py (every frame certified on the rule's own path, so that the GPU
tests may demand equal shifts everywhere), the host helpers that size the input, the cfg keys, and the build flags."""
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _stretch_ref import (D, HS, LONG_RATIOS, N, SMALL_RATIOS, T_SMALL, certified, check_shifts, frames, long_case, music,
                          position, small_cases, stretch_f32, stretch_f64, tie_case, winner)
from grafp_amd import ops
from grafp_amd.modules.transformations import GPUTransformNeuralfp
from grafp_amd.util import load_config


# ---- the rule ------------------------------------------------------------------------------------------------------
def test_window_halves_sum_to_one_and_frames_cover_every_output_twice():
    w = np.sin(np.pi * np.arange(N) / N) ** 2
    assert np.abs(w[:HS] + w[HS:] - 1).max() <= 1e-15 and w[0] == 0          # a few ulp: two rounded squares
    for T_out in (1, 255, 256, 257, 1300, 16000):
        F = frames(T_out)
        assert F == ops.stretch_frames(T_out) == int(np.ceil(T_out / HS)) + 1
        cover = np.zeros(T_out, dtype=int)
        for i in range(F):
            lo, hi = max((i - 1) * HS, 0), min((i + 1) * HS, T_out)
            cover[lo:hi] += 1
        assert (cover == 2).all()


@pytest.mark.parametrize("off", (0, 300))
def test_ratio_one_without_the_copy_branch_is_the_input_once_the_shifts_are_zero(off):
    """w[n] + w[n + HS] = 1 and at delta = 0 both frames read the same samples: the overlap-add of the rule reproduces
    xz[x_offset + m] to rounding.  (Its own winners need not be 0: the correlation is not normalised.)"""
    x = music(2000, 3)
    T_out = 1300
    got = stretch_f64(x, 1.0, T_out, off, shifts=np.zeros(frames(T_out), dtype=int), copy_at_one=False)
    want = np.zeros(T_out)
    want[:min(T_out, 2000 - off)] = x[off:off + T_out]
    assert np.abs(got.out - want).max() <= 1e-12
    copy = stretch_f64(x, 1.0, T_out, off)
    assert np.array_equal(copy.out, want) and not copy.shifts.any()
    assert np.array_equal(stretch_f32(x, 1.0, T_out, off, copy.shifts), want.astype(np.float32))


def test_a_sine_keeps_its_frequency_and_its_amplitude():
    """440 Hz at fs = 16 000 stretched at 1.06: the spectrum's peak stays in the 440 Hz bin and the amplitude at 1 -- the
    pitch is kept, which is what separates this from ops.speed_change."""
    T_out = 16000
    pad, T_in = ops.stretch_pad(1.06), ops.stretch_input_len(T_out, 1.06)
    x = np.sin(2 * np.pi * 440 * np.arange(T_in) / 16000.0)
    got = stretch_f64(x, float(np.float32(1.06)), T_out, pad)
    assert int(np.abs(np.fft.rfft(got.out * np.hanning(T_out))).argmax()) == 440
    assert abs(np.abs(got.out[1000:15000]).max() - 1) <= 2e-3
    assert np.abs(got.shifts).max() > 0                                        # it did splice


def test_tie_break_prefers_the_smaller_shift_then_the_negative_one():
    c = np.zeros(2 * D)
    assert winner(c) == 0
    c[[D - 5, D + 5, D + 9]] = 1.0
    assert winner(c) == -5
    c[D + 3] = 1.0
    assert winner(c) == 3
    c[0] = 2.0
    assert winner(c) == -D


def test_positions_are_exact_in_f64_and_not_in_f32():
    """(i - 1) * HS * rho with an f32 rho has at most 47 significant bits up to 2^30 outputs: the f64 product and the
    sum with 0.5 are exact.  An f32 product is rounded to 1/32 sample beyond frame 1024 and lands on the other side of a
    rounding boundary now and then: at rho = 0.97 from frame 1065 on, every 25th frame (not at 1.06 or 0.94 before frame
    1250, which is why the long case of the GPU tests carries a row at 0.97)."""
    from fractions import Fraction
    for r in (1.06, 0.94, 0.97, 0.5, 2.0, float(np.nextafter(np.float32(2), np.float32(0)))):
        r = float(np.float32(r))
        for i in (0, 1, 2, 700, 1100, 1249, 1 << 22):
            exact = Fraction((i - 1) * HS) * Fraction(r) + Fraction(1, 2)
            assert position(i, r, 7) == 7 + exact.numerator // exact.denominator
    f32 = lambda i, r: int(np.floor(np.float32((i - 1) * HS) * np.float32(r) + np.float32(0.5)))
    off = [i for i in range(1, 1250) if f32(i, 0.97) != position(i, float(np.float32(0.97)), 0)]
    assert off[:3] == [1065, 1090, 1115] and len(off) == 8
    assert position(0, 2.0, 700) == 700 - 512 and position(1, 1.37, 5) == 5


# ---- the condition on the GPU tests' inputs -------------------------------------------------------------------------
def _margin(ref):
    return float((ref.lead[ref.first:] / np.maximum(ref.bound[ref.first:], 1e-300)).min())


@pytest.mark.parametrize("which", ("inside", "edges"))
def test_every_frame_of_the_small_cases_is_certified(which):
    """On the rule's own path every frame's winner leads the runner-up by more than the frame's f32 bound, so a kernel
    that follows the rule has no freedom: tests/test_gpu_stretch.py demands equal shifts everywhere."""
    x, off, refs = small_cases()[which]
    for b, ref in enumerate(refs):
        ok = certified(ref)
        print(f"{which} row {b} rho={SMALL_RATIOS[b]}: shifts {ref.shifts.tolist()}, smallest lead {_margin(ref):.1f} bounds")
        assert ref.shifts.size == 7 and ok.all(), (which, b, np.flatnonzero(~ok))
        check_shifts(x[b], float(SMALL_RATIOS[b]), T_SMALL, off, ref.shifts)             # the rule passes its own check
    assert any(r.shifts.any() for r in refs)
    if which == "edges":
        assert not refs[5].out[800:].any() and np.count_nonzero(refs[5].out[:400]) > 250       # rho = 2: past the input


def test_every_frame_of_the_long_row_is_certified():
    x, T_out, refs = long_case()
    for b, ref in enumerate(refs):
        ok = certified(ref)
        print(f"long row rho={LONG_RATIOS[b]}: {ref.shifts.size} frames, smallest lead {_margin(ref):.1f} bounds")
        assert ref.shifts.size > 1100 and ok.all(), (b, np.flatnonzero(~ok))


def test_the_tie_case_ties_exactly_and_is_decided_by_the_rule():
    """Integers of period 64: candidates 64 apart have equal correlations, bit for bit, and every frame's winner is the
    one of smallest |delta| among them."""
    x, off, T_out, refs = tie_case()
    for ref in refs:
        for i in range(1, ref.shifts.size):
            c = ref.corr[i]
            assert np.array_equal(c, np.round(c)) and np.abs(c).max() < 2 ** 24
            assert np.array_equal(c[:-64], c[64:])
            assert (c == c.max()).sum() >= 4 and abs(ref.shifts[i]) <= 32
        assert ref.shifts.any()


def test_the_f32_route_stays_near_the_rule():
    """e32, the error bar's unit of tests/test_gpu_stretch.py: about 1e-7 on input of peak 1."""
    x, off, refs = small_cases()["inside"]
    for b, ref in enumerate(refs):
        e32 = np.abs(stretch_f32(x[b], SMALL_RATIOS[b], T_SMALL, off, ref.shifts) - ref.out).max()
        print(f"rho={SMALL_RATIOS[b]}: e32 = {e32:.2e}")
        assert (e32 == 0) if SMALL_RATIOS[b] == 1 else (0 < e32 < 5e-7)


# ---- the host helpers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", (0.5, 0.8, 0.94, 1.0, 1.06, 2.0))
@pytest.mark.parametrize("out_len", (1, 256, 257, 1300, 16000))
def test_stretch_input_len_keeps_every_read_inside(ratio, out_len):
    """With x_offset = stretch_pad(r) and T_in = stretch_input_len(out_len, r): at r and at ratios below it, whatever
    the shifts, no template, candidate or output read falls outside [0, T_in).  The extremes of delta are -128 and 127."""
    pad, T_in = ops.stretch_pad(ratio), ops.stretch_input_len(out_len, ratio)
    assert pad == int(np.ceil(HS * ratio)) + D + 1
    F = frames(out_len)

    def last_read(a):                  # one past: the last candidate of every frame, and the template after any shift
        return max([a[i] + D - 1 + N for i in range(1, F)] + [a[i - 1] + (D - 1 if i > 1 else 0) + HS + N for i in range(1, F)])

    for rho in sorted({ratio, float(np.float32(ratio)), max(0.5, ratio * 0.97), 0.5}):
        if rho > ratio:
            continue
        a = [position(i, rho, pad) for i in range(F)]
        lo = min([a[0] + HS] + [a[i] - D for i in range(1, F)])                 # frame 0 is only read as a template
        assert lo >= 0 and last_read(a) <= T_in, (rho, lo, last_read(a), T_in)
    if F > 2:                                                                    # and little is wasted
        assert T_in - last_read([position(i, ratio, pad) for i in range(F)]) <= 3


def test_stretch_input_len_at_the_training_shape():
    assert ops.stretch_pad(1.06) == 401 and ops.stretch_pad(2.0) == 641 and ops.stretch_pad(0.5) == 257
    assert ops.stretch_input_len(16000, 1.06) == 17867
    assert ops.stretch_input_len(ops.speed_input_len(16000, 1.06), 1.06) == 18952
    assert 18952 + 800 <= ops.DRAW_PAIRS_MAX_WINDOW == 40896


# ---- the cfg keys ---------------------------------------------------------------------------------------------------
def _cfg(**kw):
    return dict(load_config(), **kw)


BOTH = {"stretch_prob": 1.0, "stretch_range": [0.94, 1.06], "speed_prob": 1.0, "speed_range": [0.94, 1.06]}


@pytest.mark.parametrize("bad", ([0.4, 1.0], [1.0, 2.1], [1.1, 1.0], [1.0], "fast", [float("nan"), 1.0]))
def test_bad_stretch_ranges_are_refused(bad):
    with pytest.raises(ValueError, match="stretch_range"):
        GPUTransformNeuralfp(_cfg(stretch_prob=0.5, stretch_range=bad), None, None, train=True)
    with pytest.raises(ValueError, match="stretch_range"):      # also while the augmentation is off
        ops.stretch_config(_cfg(stretch_range=bad))


def test_stretch_prob_needs_a_range_and_is_a_probability():
    with pytest.raises(ValueError, match="stretch_range"):
        GPUTransformNeuralfp(_cfg(stretch_prob=0.5), None, None, train=True)
    with pytest.raises(ValueError, match="stretch_prob"):
        GPUTransformNeuralfp(_cfg(stretch_prob=1.5, stretch_range=[0.9, 1.1]), None, None, train=True)
    for off in ({}, {"stretch_prob": 0}, {"stretch_prob": 0.0, "stretch_range": [0.94, 1.06]}, {"stretch_range": [0.94, 1.06]}):
        t = GPUTransformNeuralfp(_cfg(**off), None, None, train=True)
        assert t.stretch is None and t.pad == 0 and t.draw_len == 16000 and ops.stretch_config(_cfg(**off)) is None
    t = GPUTransformNeuralfp(_cfg(stretch_prob=0.5, stretch_range=[0.94, 1.06]), None, None, train=True)
    assert t.stretch == (0.5, 0.94, 1.06) and t.speed is None
    assert (t.pad, t.stretch_pad, t.speed_pad, t.speed_len, t.draw_len, t.clip) == (401, 401, 0, 16000, 17867, 16000)


def test_both_augmentations_compose_their_lengths():
    t = GPUTransformNeuralfp(_cfg(**BOTH), None, None, train=True)
    assert (t.stretch_pad, t.speed_pad, t.pad, t.speed_len, t.draw_len) == (401, 8, 409, 16976, 18952)
    assert t.draw_len == ops.stretch_input_len(ops.speed_input_len(16000, 1.06), 1.06)
    s = GPUTransformNeuralfp(_cfg(speed_prob=1.0, speed_range=[0.94, 1.06]), None, None, train=True)     # speed alone: as before
    assert (s.stretch, s.pad, s.speed_pad, s.speed_len, s.draw_len) == (None, 8, 8, 16976, 16976)


def test_shipped_config_has_no_stretch_keys():
    cfg = load_config()
    assert "stretch_prob" not in cfg and "stretch_range" not in cfg


@pytest.mark.parametrize("shape_i,shape_j", (((4, 16000), (4, 16000)), ((4, 17867), (4, 16000)), ((4, 17866), (4, 17866)),
                                             ((17867,), (17867,))))
def test_forward_refuses_a_wrong_view_length_and_names_draw_len(shape_i, shape_j):
    t = GPUTransformNeuralfp(_cfg(stretch_prob=1.0, stretch_range=[0.94, 1.06]), None, None, train=True)
    with pytest.raises(ValueError, match=r"stretch augmentation is on.*draw_len = 17867"):
        t(torch.zeros(shape_i), torch.zeros(shape_j))
    both = GPUTransformNeuralfp(_cfg(**BOTH), None, None, train=True)
    with pytest.raises(ValueError, match=r"stretch and speed augmentation is on.*draw_len = 18952"):
        both(torch.zeros(shape_i), torch.zeros(shape_j))


def test_time_stretch_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.time_stretch(torch.zeros(2, 1000), torch.ones(2), 500)


def test_entry_reports_argument_errors_without_a_gpu():
    from grafp_amd._lib import lib
    one = 1 << 12                                            # any non-null address: the checks come before the launch
    assert lib.grafp_time_stretch_f32(None, 10, 1, 10, 0, one, one, 10, 10, None, 0, None) == -1
    assert b"null pointer" in lib.grafp_last_error()
    for args, what in (((one, 10, 0, 10, 0, one, one * 2, 10, 10, None, 0, None), b"bad sizes"),
                       ((one, 10, 1, 10, 0, one, one * 2, 1 << 31, (1 << 30) + 1, None, 0, None), b"bad sizes"),
                       ((one, 9, 1, 10, 0, one, one * 2, 10, 10, None, 0, None), b"row strides"),
                       ((one, 10, 1, 10, 0, one, one * 2, 9, 10, None, 0, None), b"row strides"),
                       ((one, 10, 1, 10, 0, one, one * 2, 300, 300, one * 3, 2, None), b"shift row stride"),
                       ((one, 10, 1, 10, 0, one, one, 10, 10, None, 0, None), b"alias"),
                       ((one, 10, 1, 10, -1, one, one * 2, 10, 10, None, 0, None), b"x_offset"),
                       # two faults at once: the checks shared with speed_change (csrc/clipwarp.h) come before the shift's
                       ((one, 300, 1, 300, 0, one, one, 300, 300, one * 3, 2, None), b"alias"),
                       ((one, 300, 1, 300, -1, one, one * 2, 300, 300, one * 3, 2, None), b"x_offset")):
        assert lib.grafp_time_stretch_f32(*args) == -1 and what in lib.grafp_last_error(), what


def test_stretch_kernel_has_no_packed_f32_and_reads_lds_wide():
    """The shipped object's own command (make -n), compiled to device assembly: no packed-f32 instruction at all in
    stretch.hip; the correlations are fma chains fed by 16-byte LDS reads; no scratch."""
    asm = shipped_asm("stretch")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert any("time_stretch_kernel" in k for k in kernels)
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm
    assert "ds_read_b128" in asm
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", asm)
