"""CPU tests of what the k-NN graph GPU tests stand on (tests/_knn_ref.py): the C oracle (oracle/csrc/knn_graph.c, the
bit-for-bit contract of the three kernel files) meets both float64 rules on every case, the equality rule covers all but
a capped share of an unstructured clip, the planted queries land in the tiers they were planted for, and the plan and
workspace queries of knn_split.hip / knn_pre.hip (pure host functions: no GPU) answer what the case table claims."""
import numpy as np
import pytest

import _knn_ref as kr

ALL_CASES = kr.CASES + kr.PRE_CASES
DT_CODE = {"f32": 0, "bf16": 1}


def _lib():
    from grafp_amd._lib import lib
    return lib


@pytest.mark.parametrize("dtype", kr.DTYPES)
@pytest.mark.parametrize("c", ALL_CASES + [kr.UNSUPPORTED], ids=kr.case_id)
def test_c_oracle_meets_both_rules_and_the_cap_holds(c, dtype):
    """k = 1 and 4.  The cap (0.04 of the unstructured clip's queries, 0.10 at C = 992) is asserted so that a change of
    tol() cannot hollow the equality rule out; with one clip only, over that clip's queries that were not planted."""
    from oracle import native
    x, ref = kr.inputs(c, dtype), kr.cached_ref(c, dtype)
    for k in kr.K_CPU:
        v = kr.check(native.knn_graph(x, k), ref, c.C, f"oracle {kr.case_id(c)} {dtype} k={k}")
        assert v.ratio <= 0.5, "the oracle's own rounding is bounded by half the bar"
        sep = kr.separated(ref, k, kr.tol(c.C))
        if kr.plain_clip(c) is not None:
            share = 1.0 - float(sep[kr.plain_clip(c)].mean())
        else:
            keep = np.ones(c.N, bool)
            keep[[q for _, q in kr.planted(c)]] = False
            share = 1.0 - float(sep[0][keep].mean())
        print(f"knn {kr.case_id(c)} {dtype} k={k}: the equality rule leaves out {share:.4f} of the unstructured queries")
        assert share <= kr.cap(c.C), (k, share)


def test_planted_ties_are_exact_and_go_to_the_lowest_index():
    """The float64 distances among copies of a column are exactly 0, so the reference itself states the tie rule: the
    triple's members list each other in index order, and so does the C oracle."""
    from oracle import native
    c = kr.CASES[2]
    x, ref = kr.inputs(c, "f32"), kr.cached_ref(c, "f32")
    bc, bt, bp = kr.structure_clips(c)
    trip = kr.triple_cols(c.N)
    want = native.knn_graph(x, 3)
    for q in trip:
        assert np.array_equal(ref.ds[bt, q, :3], np.zeros(3)) and ref.ds[bt, q, 3] > 0.1
        assert tuple(ref.order[bt, q, :3]) == trip == tuple(want[bt, q])
        assert set(ref.same[bt, list(trip)]) == {trip[0]}
    for q in kr.PAIR_COLS:
        assert tuple(ref.order[bp, q, :2]) == kr.PAIR_COLS == tuple(want[bp, q, :2])
    assert np.array_equal(ref.same[kr.plain_clip(c)], np.arange(c.N))
    # bf16: rounding keeps copies equal and the cluster distinct enough to be a cluster, not one node
    xb = kr.inputs(c, "bf16")
    assert np.array_equal(kr.to_bf16(xb), xb) and np.array_equal(xb[bt, :, trip[0]], xb[bt, :, trip[2]])
    assert len({xb[bc, :, q].tobytes() for q in kr.CLUSTER_COLS}) > 20


@pytest.mark.parametrize("dtype", kr.DTYPES)
@pytest.mark.parametrize("c", [c for c in ALL_CASES if c.N <= 640], ids=kr.case_id)
def test_planted_queries_land_in_both_exact_passes(c, dtype):
    """In float64, with decided gaps only (under a tenth of the band 2 m(C) or over ten times it): every row holds a
    surely-LIGHT and a surely-HEAVY planted query (f32: at each of k = 1, 3 and 4; bf16, whose cluster is ten times wider:
    surely-HEAVY at k = 1 at least), the triple is HEAVY at k = 1 (three candidates at distance 0) and LIGHT at k = 3, and
    the exact copies are uncertified at every k."""
    ref, bnd = kr.cached_ref(c, dtype), kr.band(c.C, dtype)
    bc, bt, bp = kr.structure_clips(c)
    row_light = row_heavy = 0
    for k in kr.K_GPU:
        unc, light, heavy = kr.sure_tiers(ref, k, bnd)
        qs = kr.planted(c)
        n_light, n_heavy = sum(int(light[b, q]) for b, q in qs), sum(int(heavy[b, q]) for b, q in qs)
        print(f"knn {kr.case_id(c)} {dtype} k={k}: planted queries surely LIGHT {n_light}, surely HEAVY {n_heavy}, "
              f"surely uncertified {kr.sure_uncertified_planted(c, dtype, k)} of {len(qs)}")
        row_light, row_heavy = row_light + n_light, row_heavy + n_heavy
        assert n_light >= 1 and (n_heavy >= 1 or dtype == "bf16"), (k, n_light, n_heavy)
        for q in kr.triple_cols(c.N):                              # (at k = 4 the tier hangs on an unplanted gap)
            assert unc[bt, q] and (heavy[bt, q] if k == 1 else light[bt, q] if k == 3 else True)
        for q in kr.PAIR_COLS:
            assert unc[bp, q] and (light[bp, q] or k > 1)
        if dtype == "f32":                                         # 1e-3 is far inside the band; bf16's 1e-2 need not be
            assert all(heavy[bc, q] for q in kr.CLUSTER_COLS)
        assert kr.sure_uncertified_planted(c, dtype, k) >= 5
    assert row_light >= 1 and row_heavy >= 3                       # bf16: at least the triple at k = 1


def test_all_heavy_clips_in_float64():
    ref = kr.make_ref(kr.heavy_clips())
    assert not ref.d[0].any() and np.array_equal(ref.order[0, :, :4], np.tile(np.arange(4), (640, 1)))
    assert set(np.unique(ref.d[1])) == {0.0, 2.0}
    for k in (1, 3, 4):
        assert kr.sure_tiers(ref, k, kr.band(64, "f32"))[2].all()  # every query HEAVY
    from oracle import native
    kr.check_exact(native.knn_graph(kr.heavy_clips(), 4), ref, "oracle, all-HEAVY clips")


@pytest.mark.parametrize("C,N,B", [(64, 640, 3), (96, 384, 3), (40, 300, 2)])
def test_c_oracle_on_integer_features_is_the_stable_argsort(C, N, B):
    from oracle import native
    x = kr.int_inputs(C, N, B)
    ref = kr.make_ref(x, normalize=False)
    assert np.array_equal(ref.d, np.round(ref.d)) and (np.diff(ref.ds, axis=-1) == 0).any()      # integers, with ties
    for k in (1, 4, 8):
        kr.check_exact(native.knn_graph(x, k, normalize=False), ref, f"oracle int {C}-{N} k={k}")


def test_reference_rejects_a_wrong_neighbour_and_a_swapped_near_tie_only_where_decided():
    """The rules bite: a neighbour from outside the true set, a repeated index, an index >= N and a swap of two well
    separated neighbours each fail; a swap inside the bar does not."""
    c = kr.CASES[0]
    ref = kr.cached_ref(c, "f32")
    good = ref.order[..., :3].copy()
    assert kr.judge(good, ref, c.C)[:4] == (0.0, True, True, 0)
    b = c.B - 1
    q = int(np.argmax(kr.separated(ref, 3, kr.tol(c.C))[b]))
    for mutate, field in ((lambda a: a.__setitem__((b, q, 2), ref.order[b, q, 9]), "ratio"),
                          (lambda a: a.__setitem__((b, q, 2), a[b, q, 1]), "distinct"),
                          (lambda a: a.__setitem__((b, q, 2), c.N), "in_range"),
                          (lambda a: a.__setitem__((b, q), a[b, q, [0, 2, 1]]), "mismatches")):
        bad = good.copy()
        mutate(bad)
        v = kr.judge(bad, ref, c.C)
        assert {"ratio": v.ratio > 1.0, "distinct": not v.distinct, "in_range": not v.in_range,
                "mismatches": v.mismatches == 1}[field], field


# ---- the plan queries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL_CASES + [kr.UNSUPPORTED], ids=kr.case_id)
def test_plan_queries_answer_what_the_case_table_claims(c):
    lib = _lib()
    for k in (1, 2, 3, 4):
        assert lib.grafp_knn_split_supported(c.C, c.N, k) == (0 if c is kr.UNSUPPORTED else 1)
        assert lib.grafp_knn_split_preferred_for(0, c.C, c.N, k) == c.pref_f32 == lib.grafp_knn_split_preferred(c.C, c.N, k)
        assert lib.grafp_knn_split_preferred_for(1, c.C, c.N, k) == c.pref_bf16
        assert lib.grafp_knn_pre_supported(c.C, c.N, k) == c.pre
    assert lib.grafp_knn_split_supported(c.C, c.N, 5) == 0 == lib.grafp_knn_pre_supported(c.C, c.N, 5)
    # the rule of the table's columns: f32 inputs up to 128 channels, bf16 inputs up to 256, the pre-filter C % 64 == 0
    assert c.pref_f32 == int(c.C <= 128) and c.pref_bf16 == int(c.C <= 256) and c.pre == int(c.C % 64 == 0)


def test_split_support_ends_at_992_channels_and_keeps_the_ragged_clip_lengths():
    """C = 992 is the last supported multiple of 32 (ks_margin(1024) exceeds 0.9 * 2^-10).  A clip length that is a
    multiple of 128 but not of 512 stays supported: pass 3b bounds its last column range (it used to run 512 columns
    from N - N % 512 on, into the next clip)."""
    lib = _lib()
    assert [C for C in range(32, 2049, 32) if lib.grafp_knn_split_supported(C, 128, 3)] == list(range(32, 993, 32))
    assert [N for N in range(64, 4500, 64) if lib.grafp_knn_split_supported(64, N, 3)] == list(range(128, 4097, 128))
    for N in (640, 768, 896, 1152, 1664):
        assert lib.grafp_knn_split_supported(64, N, 4) == 1 and lib.grafp_knn_split_preferred_for(0, 64, N, 4) == 1
        assert lib.grafp_knn_split_preferred_for(1, 256, N, 4) == 1
    # the encoder's own stages
    for C, N in ((64, 1024), (128, 512), (256, 256), (512, 128)):
        assert lib.grafp_knn_split_supported(C, N, 3) == 1
        assert lib.grafp_knn_split_preferred_for(0, C, N, 3) == int(C <= 128)
        assert lib.grafp_knn_split_preferred_for(1, C, N, 3) == int(C <= 256)
        assert lib.grafp_knn_pre_supported(C, N, 3) == 1


@pytest.mark.parametrize("c", ALL_CASES + [kr.UNSUPPORTED], ids=kr.case_id)
def test_workspace_queries_are_positive_multiples_of_16(c):
    lib = _lib()
    nodes = c.B * c.N
    sizes = {
        "split f32": lib.grafp_knn_split_workspace_for(0, c.B, c.C, c.N),
        "split bf16": lib.grafp_knn_split_workspace_for(1, c.B, c.C, c.N),
        "pre": lib.grafp_knn_pre_workspace(c.B, c.C, c.N),
        "exact": lib.grafp_knn_graph_workspace(c.B, c.C, c.N),
    }
    for name, n in sizes.items():
        assert n > 0 and n % 16 == 0, (name, n)
    assert sizes["split f32"] == lib.grafp_knn_split_workspace(c.B, c.C, c.N)
    # what each layout must at least hold: norms and denominators, the two bf16 planes or the candidate table, flags,
    # the LIGHT pass's extra candidate
    assert sizes["split f32"] >= nodes * (4 + 4 + 1 + 4) + 2 * 2 * nodes * c.C
    assert sizes["split bf16"] >= nodes * (4 + 4 + 8 + 1 + 4)
    assert sizes["pre"] >= nodes * c.C * 6 + nodes * 4 and sizes["exact"] >= nodes * c.C * 4 + nodes * 4
    assert lib.grafp_knn_split_workspace_for(0, 0, c.C, c.N) == 0
