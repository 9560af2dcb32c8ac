"""CPU tests of what the augmentation GPU tests stand on (tests/_augment_ref.py): the float64 references and their derived
bars against the C oracle (oracle/csrc/augment.c), the kernel constants against grafp_amd/csrc/augment.hip, the planted
defects against the bars, and the case tables against what they claim to reach.  No GPU."""
import os
import re

import numpy as np
import pytest

import _augment_ref as ar

_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grafp_amd", "csrc", "augment.hip")


def test_constants_are_the_kernels():
    """Every `constexpr int NAME = expression;` of augment.hip, evaluated in file order: the restated ones are equal, so a
    retuned tile cannot leave the case tables on yesterday's seams."""
    with open(_HIP) as f:
        found = re.findall(r"^constexpr int (\w+) = ([^;]+);", f.read(), flags=re.M)
    values = {}
    for name, expr in found:
        assert re.fullmatch(r"[\w\s+\-*/()]+", expr), (name, expr)
        values[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(values)))
    for name, want in ar.KERNEL_CONSTANTS.items():
        assert values.get(name) == want, (name, values.get(name), want)


@pytest.mark.parametrize("name", [c.name for c in ar.CONV_CASES])
def test_convolution_oracle_lies_within_the_bar(name):
    """oracle.native.ir_convolve (one fmaf chain per output: the order the kernel reproduces) against float64, per output
    on every clip, ragged and padded bank alike; the skipped clip is its input, bit for bit."""
    from oracle import native as on
    (x, recs, idx), _ = ar.cached_conv(name)
    flat, starts, lens = ar.ragged(recs)
    got = on.ir_convolve(x, flat, lens, idx, starts)
    assert np.array_equal(got.view(np.uint32), on.ir_convolve(x, ar.padded(recs), lens, idx).view(np.uint32))
    assert np.array_equal(got[-1].view(np.uint32), x[-1].view(np.uint32))
    ratio = ar.conv_excess(got, name)
    print(f"augment-bar conv oracle {name}: worst error / bar {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", [c.name for c in ar.MIX_CASES])
def test_mix_oracle_lies_within_the_bar(name):
    """oracle.native.mix_snr (double sums, one f32 scale, one fmaf per sample) against float64 on every clip."""
    from oracle import native as on
    (x, recs, idx, off, snr), _ = ar.cached_mix(name)
    flat, starts, lens = ar.ragged(recs)
    got = on.mix_snr(x, flat, lens, idx, off, snr, starts)
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), on.mix_snr(x, ar.padded(recs), lens, idx, off, snr).view(np.uint32))
    assert np.array_equal(got[-1].view(np.uint32), x[-1].view(np.uint32))
    if ar.MIX_BY_NAME[name].kind in ("zero-signal", "zero-noise"):
        assert np.array_equal(got, x)
    ratio = ar.mix_excess(got, name)
    print(f"augment-bar mix oracle {name}: worst error / bar {ratio:.3f}")
    assert ratio <= 1.0


def test_quiet_recording_makes_the_1e_8_visible():
    (_, recs, _, _, _), _ = ar.cached_mix("quiet-recording")
    rms = float(np.sqrt((recs[1].astype(np.float64) ** 2).mean()))
    assert 0.08 < 1e-8 / (rms + 1e-8) < 0.12


@pytest.mark.parametrize("defect", ar.CONV_DEFECTS)
def test_planted_convolution_defects_leave_the_bar(defect):
    seen = ar.assert_defect_shows(ar.conv_defect_excess, defect, [c.name for c in ar.CONV_CASES])
    print(f"augment-defect conv {defect}: " + ", ".join(f"{k} {v:.3g}" for k, v in seen.items()))


@pytest.mark.parametrize("defect", ar.MIX_DEFECTS)
def test_planted_mix_defects_leave_the_bar(defect):
    must = ("quiet-recording",) if defect == "no-1e-8" else ()
    seen = ar.assert_defect_shows(ar.mix_defect_excess, defect, [c.name for c in ar.MIX_CASES], must)
    print(f"augment-defect mix {defect}: " + ", ".join(f"{k} {v:.3g}" for k, v in seen.items()))


@pytest.mark.parametrize("name", [c.name for c in ar.CONV_CASES])
def test_convolution_cases_reach_what_they_claim(name):
    """Tiles, outputs of the last tile and of its .y halves, and per recording and tile the side of the l_end clamp, the
    chunks walked and the taps of the last chunk: recomputed from the constants."""
    case = ar.CONV_BY_NAME[name]
    assert set(case.reach) == set(case.Ls)
    for L in case.Ls:
        tiles, last, upper, per_tile = ar.conv_reach(case.T, L)
        assert (tiles, last, upper) == (case.tiles, case.last, case.upper), (L, tiles, last, upper)
        assert per_tile == case.reach[L], (L, per_tile)


def test_convolution_table_sits_on_every_seam():
    """What the table as a whole must reach, stated on conv_reach's terms."""
    reach = {(c.name, L): ar.conv_reach(c.T, L) for c in ar.CONV_CASES for L in c.Ls}
    every_tile = [(c, L, k, t) for (c, L), r in reach.items() for k, t in enumerate(r[3])]
    assert any(r[0] > 1 and r[1] == 1 for r in reach.values())                         # a last tile of one output
    assert any(r[2] == 1 for r in reach.values())                                      # one output in the .y halves
    assert any(r[1] == ar.AC_TT and r[0] > 1 for r in reach.values())                  # full tiles only, more than one
    assert {ar.AC_LC - 1, ar.AC_LC, ar.AC_LC + 1, ar.AC_R, ar.AC_R + 1, 1} <= {L for _, L in reach}
    # L = t0 + AC_TT, where the clamp's two sides meet: on the first tile and on a later one
    assert any(side == "tile" and L == ar.AC_TT for _, L, k, (side, _, _) in every_tile if k == 0)
    assert any(side == "tile" and L == (k + 1) * ar.AC_TT for _, L, k, (side, _, _) in every_tile if k >= 1)
    assert any(len({side for side, _, _ in r[3]}) == 2 for r in reach.values())        # the side changes inside a clip
    assert any(taps < ar.AC_LC for _, _, _, (_, _, taps) in every_tile)               # a zero-padded chunk
    assert any(L > ar.CONV_BY_NAME[c].T for c, L in reach) and any(L == ar.CONV_BY_NAME[c].T for c, L in reach)


@pytest.mark.parametrize("name", [c.name for c in ar.MIX_CASES])
def test_mix_cases_reach_what_they_claim(name):
    case = ar.MIX_BY_NAME[name]
    assert ar.mix_reach(case.T, case.nl) == (case.chunks, case.last, case.step)
    x, recs, idx, off, snr = ar.mix_inputs(case)
    assert recs[1].size == case.nl and list(idx) == [1, 1, 1, 1, -1] and [float(s) for s in snr[:4]] == [-5.0, 0.0, float(np.float32(7.3)), 30.0]
    assert (off >= 0).all() and x.shape == (5, case.T)


def test_mix_table_sits_on_every_seam():
    cs = ar.MIX_CASES
    assert {1, 2, ar.MX_THREADS - 1, ar.MX_THREADS, ar.MX_THREADS + 1, ar.MX_CHUNK} <= {c.nl for c in cs}
    assert any(c.nl == c.T for c in cs) and any(c.nl > c.T for c in cs) and any(c.off == c.nl - 1 for c in cs)
    assert any(c.off >= c.nl for c in cs) and any(c.step == 0 and c.nl > 1 for c in cs) and any(c.step == 1 for c in cs)
    assert any(c.chunks > 1 and c.last == 1 for c in cs) and any(c.chunks == 1 and c.last == ar.MX_CHUNK for c in cs)
    assert {"quiet", "zero-signal", "zero-noise"} <= {c.kind for c in cs}
