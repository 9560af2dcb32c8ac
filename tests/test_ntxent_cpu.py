"""CPU tests of what the NT-Xent GPU tests stand on (tests/_ntxent_ref.py): the float64 reference against the reference
project's own outputs, the local form against the global one, and the launch plan of ntxent.hip through grafp_ntxent_plan
(a pure host function: no GPU) -- every regime of the split rule is reached by a case of the GPU tests' table, and no
plan needs more workspace than grafp_ntxent_workspace reports."""
import ctypes

import numpy as np
import pytest

import _ntxent_ref as nr
from _common import golden

ALL_CASES = nr.FULL_CASES + nr.LOCAL_CASES


def _lib():
    from grafp_amd._lib import lib
    return lib


def _plan_of(c):
    return nr.plan(_lib(), c.B, c.n_local if isinstance(c, nr.Local) else c.B)


@pytest.mark.parametrize("B", [2, 8, 32])
def test_reference_matches_the_reference_projects_outputs(B):
    """tests/golden/ntxent.npz holds f32 results at tau = 0.05: they are the side with the f32 error here, so the bars
    of _ntxent_ref apply as they stand."""
    g = golden("ntxent.npz")
    zi, zj = g[f"zi_{B}"], g[f"zj_{B}"]
    ref = nr.ntxent_f64(zi, zj, 0.05)
    sc = nr.scales(zi, zj, 0.05)
    assert nr.worst(g[f"loss_{B}"], ref.loss, nr.loss_bar(ref.loss, sc)) <= 1.0
    assert nr.worst(g[f"dzi_{B}"], ref.dzi, nr.grad_bar(ref.dzi, sc)) <= 1.0
    assert nr.worst(g[f"dzj_{B}"], ref.dzj, nr.grad_bar(ref.dzj, sc)) <= 1.0
    assert np.all(ref.lse >= ref.pos)                                  # the positive is one of the summed logits


def test_reference_degenerate_and_duplicate_inputs():
    """B = 1: the only candidate is the partner, so the loss and the gradients are exactly 0.  dup: the positive logit is
    the row's squared norm / tau, the largest logit of its row."""
    r = nr.cached_ref(1, 32, 0.05, "unit")
    assert r.loss == 0.0 and not r.dzi.any() and not r.dzj.any()
    zi, zj = nr.inputs(70, 64, "dup")
    assert np.array_equal(zi, zj) and np.array_equal(zi[3], zi[1])
    r = nr.cached_ref(70, 64, 0.05, "dup")
    S = np.concatenate([zi, zj]).astype(np.float64) @ np.concatenate([zi, zj]).astype(np.float64).T / 0.05
    np.fill_diagonal(S, -np.inf)
    assert np.allclose(r.pos, S.max(axis=1), rtol=0, atol=1e-12)
    zi, zj = nr.inputs(300, 64, "norms")
    ni, nj = np.linalg.norm(zi, axis=1), np.linalg.norm(zj, axis=1)
    assert np.allclose(ni * nj, 1.0, atol=1e-5) and abs(np.log(ni[-1]) - 0.7) < 1e-5 and abs(np.log(nj[0]) - 0.7) < 1e-5


@pytest.mark.parametrize("B,D,tau,kind,parts", [
    (520, 128, 0.05, "unit", nr.PARTITION_520),
    (33, 128, 0.05, "unit", [(0, 32), (32, 1)]),
    (193, 64, 0.1, "norms", [(0, 17), (17, 50), (67, 126)])])
def test_local_shares_add_up_and_local_gradients_are_slices(B, D, tau, kind, parts):
    ref = nr.cached_ref(B, D, tau, kind)
    assert parts[0][0] == 0 and sum(n for _, n in parts) == B
    total, v = 0.0, ref.lse - ref.pos
    for lo, n in parts:
        loc = nr.local_f64(ref, lo, n)
        total += loc.share
        assert np.array_equal(loc.dzi, ref.dzi[lo:lo + n]) and np.array_equal(loc.dzj, ref.dzj[lo:lo + n])   # exactly
        assert len(loc.partials) == 2 * ((n + 31) // 32)
        assert abs(loc.partials.sum() / (2 * B) - loc.share) <= 1e-13 * max(1.0, abs(loc.share))
        nb = len(loc.partials) // 2
        assert loc.partials[0] == v[lo:lo + min(32, n)].sum() and loc.partials[nb] == v[B + lo:B + lo + min(32, n)].sum()
    assert abs(total - ref.loss) <= 1e-12 * abs(ref.loss)


def test_case_table_reaches_every_regime_of_the_plan():
    """Each regime of the split rule, stated on what grafp_ntxent_plan reports (not on a restatement of the rule)."""
    seen = {}
    for c in ALL_CASES:
        p = _plan_of(c)
        M, per, per2 = 2 * c.B, p.rows // nr.NT_C, p.rows2 // nr.NT_C
        assert p.chunks == (M + nr.NT_C - 1) // nr.NT_C and p.rows == per * nr.NT_C and p.rows2 == per2 * nr.NT_C
        assert p.splits * p.rows >= M and p.splits2 * p.rows2 >= M, "the splits must cover every candidate row"
        assert 1 <= p.splits2 <= p.splits <= 8
        e1, e2 = nr.empty_splits(p.chunks, p.splits, p.rows), nr.empty_splits(p.chunks, p.splits2, p.rows2)
        tail = M % nr.NT_C
        flags = {
            "one split": p.splits == 1,
            "several splits dealt evenly": p.splits > 1 and p.chunks == p.splits * per,
            "several splits dealt unevenly": p.splits > 1 and e1 == 0 and p.chunks != p.splits * per,
            "last chunk under 32 rows in a multi-split plan": p.splits > 1 and 0 < tail < 32,
            "one trailing empty pass-1 split": e1 == 1,
            "two trailing empty pass-1 splits": e1 == 2,
            "pass 2 split like pass 1": p.splits2 == p.splits > 1,
            "pass 2 split less than pass 1": 1 < p.splits2 < p.splits,
            "pass 2 unsplit under a split pass 1": p.splits2 == 1 < p.splits,
            "pass 2 with an empty split of its own": p.splits2 > 1 and e2 >= 1,
        }
        for k, hit in flags.items():
            if hit:
                seen.setdefault(k, []).append(nr.case_id(c))
    missing = [k for k in flags if k not in seen]
    assert not missing, missing


@pytest.mark.parametrize("B,plan", [(1, (1, 1, 128, 1, 128)), (2, (1, 1, 128, 1, 128)), (33, (1, 1, 128, 1, 128)),
                                    (129, (3, 1, 384, 1, 384)), (193, (4, 2, 256, 2, 256)), (300, (5, 2, 384, 2, 384)),
                                    (520, (9, 4, 384, 4, 384)), (577, (10, 5, 256, 5, 256)),
                                    (1100, (18, 8, 384, 3, 768)), (2049, (33, 8, 640, 1, 4224))])
def test_plan_of_the_full_form_is_the_documented_table(B, plan):
    """The regime table of DESIGN.md (chunks, pass-1 splits, rows per split, pass-2 splits, rows per split)."""
    assert tuple(nr.plan(_lib(), B, B)[:5]) == plan


@pytest.mark.parametrize("c", ALL_CASES, ids=nr.case_id)
def test_plan_fits_the_reported_workspace_and_partials(c):
    lib = _lib()
    n_local = c.n_local if isinstance(c, nr.Local) else c.B
    p = _plan_of(c)
    assert p.partials == lib.grafp_ntxent_num_partials(n_local) == 2 * ((n_local + 31) // 32)
    assert nr.plan_bytes(p, c.B, n_local, 128) <= lib.grafp_ntxent_workspace(c.B)
    # the full form at D = 128 with pass 2 split like pass 1 uses all of it: the report is not padded
    if n_local == c.B and p.splits2 == p.splits:
        assert nr.plan_bytes(p, c.B, n_local, 128) == lib.grafp_ntxent_workspace(c.B)


def test_workspace_covers_every_plan_up_to_1200_pairs():
    """Beyond the table: any local range of any B_all <= 1200 at D = 128 (n_local only enters through its block count)."""
    lib = _lib()
    for B in range(1, 1201):
        ws = lib.grafp_ntxent_workspace(B)
        for n_local in sorted({1, B} | set(range(32, B + 1, 32))):
            assert nr.plan_bytes(nr.plan(lib, B, n_local), B, n_local, 128) <= ws, (B, n_local)


@pytest.mark.parametrize("B_all,n_local", [(0, 0), (0, 1), (-3, 1), (8, 0), (8, -1), (8, 9)])
def test_plan_refuses_bad_arguments_and_zeroes_info(B_all, n_local):
    lib = _lib()
    info = (ctypes.c_int * 8)(*([7] * 8))
    assert lib.grafp_ntxent_plan(B_all, n_local, info) != 0
    assert b"ntxent_plan" in lib.grafp_last_error()
    assert list(info) == [0] * 8
    assert lib.grafp_ntxent_plan(8, 8, None) != 0 and b"null pointer" in lib.grafp_last_error()
