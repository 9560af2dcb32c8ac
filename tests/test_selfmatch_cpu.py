"""CPU tests of shared-audio detection inside a library (csrc/selfmatch.hip, ops.self_match,
FingerprintLibrary.self_matches / duplicate_groups): the numpy restatement on hand-built cases, the refusal paths, the
C ABI entry, the shipped assembly and the command line.  No GPU call is made."""
import ctypes
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _identify_ref import identify_item, score_run
from _selfmatch_ref import self_match_ref, self_match_track
from grafp_amd import library, ops

INT_MIN = np.iinfo(np.int32).min


def _rows(n, seed):
    """Dyadic rows (multiples of 2^-8 in [-1/8, 1/8)): every product and partial sum is exact in f32."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-32, 32, size=(n, 128)) / 256.0).astype(np.float32)


def _ids(n, k, hits):
    """(n, k) ids, -1 everywhere but the listed {row: [ids]}."""
    ids = np.full((n, k), -1, np.int64)
    for r, h in hits.items():
        ids[r, :len(h)] = h
    return ids


def test_own_track_hits_are_dropped():
    first = np.array([0, 6, 12])
    rows = _rows(12, 1)
    # every row of track 0 hits its own next row (as at overlap 0.9) and its copy in track 1 at delta 0
    ids = _ids(12, 2, {i: [min(i + 1, 5), 6 + i] for i in range(6)})
    res = self_match_track(rows, first, ids, 0, min_votes=1)
    assert [(b, d, lo, m, v) for b, d, lo, m, _, v in res] == [(1, 0, 0, 6, 6)]
    assert self_match_track(rows, first, _ids(12, 2, {i: [i, 5 - i] for i in range(6)}), 0, min_votes=1) == []


def test_span_is_taken_from_the_min_and_max_voting_rows():
    first = np.array([0, 10, 30])
    rows = _rows(30, 2)
    # rows 2, 5 and 7 of track 0 hit track 1 at delta 4 (rows 6, 9, 11 of track 1 = global 16, 19, 21)
    ids = _ids(30, 3, {2: [16], 5: [19, -1, 3], 7: [21]})
    (b, d, lo, m, sc, v), = self_match_track(rows, first, ids, 0, min_votes=3)
    assert (b, d, lo, m, v) == (1, 4, 2, 6, 3)
    # the score runs over every row of the span, voting or not
    assert sc == score_run(rows[2:8], rows[16:22])


def test_best_delta_per_pair_and_score_ties_go_to_the_smaller_delta():
    base = _rows(3, 3)
    other = _rows(3, 4)
    first = np.array([0, 3, 12])
    rows = np.concatenate([base, other, base, base])            # track 1 = other + base + base
    ids = _ids(12, 2, {0: [6, 9], 1: [7, 10], 2: [8, 11]})      # track 0 aligns at delta 3 and delta 6: equal scores
    res = self_match_track(rows, first, ids, 0, min_votes=3)
    assert [(b, d, v) for b, d, _, _, _, v in res] == [(1, 3, 3)]
    ids2 = _ids(12, 2, {0: [3, 6], 1: [4, 7], 2: [5, 8]})      # delta 0 (the other rows) scores lower than delta 3
    res2 = self_match_track(rows, first, ids2, 0, min_votes=3)
    assert [(b, d) for b, d, _, _, _, _ in res2] == [(1, 3)]
    assert res2[0][4] == score_run(base, base)


def test_min_votes_and_min_overlap_filters():
    first = np.array([0, 8, 16])
    rows = _rows(16, 5)
    ids = _ids(16, 1, {0: [8], 1: [9], 5: [13]})                # 3 votes over a span of 6 rows
    assert len(self_match_track(rows, first, ids, 0, min_votes=3, min_overlap=6)) == 1
    assert self_match_track(rows, first, ids, 0, min_votes=4, min_overlap=1) == []
    assert self_match_track(rows, first, ids, 0, min_votes=3, min_overlap=7) == []


def test_ordering_by_score_then_track():
    base = _rows(4, 6)
    noise = _rows(4, 7)
    first = np.array([0, 4, 8, 12, 16])
    rows = np.concatenate([base, noise * 0 + base * 0.5, base, base])     # tracks 2 and 3 equal 0, track 1 half
    ids = _ids(16, 3, {i: [4 + i, 8 + i, 12 + i] for i in range(4)})
    res = self_match_track(rows, first, ids, 0, min_votes=4)
    assert [b for b, *_ in res] == [2, 3, 1]
    assert res[0][4] == res[1][4] > res[2][4]
    assert [b for b, *_ in self_match_track(rows, first, ids, 0, top=2, min_votes=4)] == [2, 3]


def test_zero_row_tracks_minus_one_and_duplicate_ids():
    first = np.array([0, 0, 5, 5, 10, 10])
    rows = _rows(10, 8)
    ids = _ids(10, 3, {0: [5, 5, -1], 1: [6, 99, -7], 2: [7, -1, -1]})
    res = self_match_track(rows, first, ids, 1, min_votes=4)
    assert [(b, d, lo, m, v) for b, d, lo, m, _, v in res] == [(3, 0, 0, 3, 4)]
    b_, d_, lo_, m_, sc_, v_ = self_match_ref(rows, first, ids, min_votes=4, top=3)
    assert b_.tolist() == [[-1, -1, -1], [3, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]]
    assert d_[0, 0] == INT_MIN and lo_[0, 0] == -1 and m_[0, 0] == 0 and np.isneginf(sc_[0, 0]) and v_[0, 0] == 0


def test_tracks_subset_equals_the_rows_of_the_full_result():
    rng = np.random.RandomState(9)
    first = np.array([0, 7, 7, 20, 31, 40])
    rows = _rows(40, 10)
    ids = rng.randint(-1, 40, size=(40, 4))
    ids[:7, 0] = np.arange(20, 27)
    full = self_match_ref(rows, first, ids, min_votes=1)
    sub = self_match_ref(rows, first, ids, tracks=[3, 0], min_votes=1)
    for f, s in zip(full, sub):
        assert np.array_equal(f[[3, 0]], s)


def test_a_span_inside_one_track_scores_as_identify():
    first = np.array([0, 12, 30])
    rows = _rows(30, 11)
    ids = _ids(30, 1, {3 + i: [15 + i] for i in range(5)})     # rows 3..7 of track 0 on rows 3..7 of track 1
    (b, d, lo, m, sc, v), = self_match_track(rows, first, ids, 0, min_votes=5)
    q = rows[3:8]
    (t, off, isc, iv), = identify_item(rows, first, q, np.arange(15, 20)[:, None])
    assert (t, off, iv) == (1, 3, 5) and (b, lo + d, v) == (1, 3, 5)
    assert sc == isc                                            # the same bits


# ---- host refusals, the ABI entry and the shipped object ---------------------------------------------------------
def test_self_match_op_refusals_without_a_gpu():
    rows = torch.zeros(8, 128)
    first = torch.tensor([0, 3, 8])
    ids = torch.zeros(8, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="k=33"):
        ops.self_match(rows, first, torch.zeros(8, 33, dtype=torch.int64))
    with pytest.raises(ValueError, match="top"):
        ops.self_match(rows, first, ids, top=65)
    with pytest.raises(ValueError, match="top"):
        ops.self_match(rows, first, ids, top=0)
    with pytest.raises(ValueError, match="at least 1"):
        ops.self_match(rows, first, ids, min_votes=0)
    with pytest.raises(ValueError, match="at least 1"):
        ops.self_match(rows, first, ids, min_overlap=0)
    with pytest.raises(ValueError, match="never decrease"):
        ops.self_match(rows, torch.tensor([0, 5, 3, 8]), ids)
    with pytest.raises(ValueError, match="rows for a library"):
        ops.self_match(rows, first, torch.zeros(7, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="source tracks"):
        ops.self_match(rows, first, ids, tracks=[2])
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.self_match(rows, first, ids)


def test_abi_entry_follows_the_conventions():
    from test_abi import _ctype_of, _declared
    from grafp_amd import _lib
    d = _declared()
    for name in ("grafp_self_match_f32", "grafp_self_match_workspace"):
        ret, args = d[name]
        res, argtypes = _lib.SIGNATURES[name]
        assert [_ctype_of(a) for a in args] == list(argtypes), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    ret, args = d["grafp_self_match_f32"]
    assert ret == "int" and args[-1].startswith("grafp_stream_t")
    assert d["grafp_self_match_workspace"][0] == "size_t"


def test_abi_entry_refuses_out_of_range_launches_without_a_gpu():
    from grafp_amd._lib import lib
    # never dereferenced: every call below fails an argument check before anything is launched
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(11)]
    ws_ok = ops.self_match_workspace_bytes([25, 25, 25, 25], 8, 4)

    def call(k=8, top=8, mv=4, mo=1, ws=ws_ok, p0=fake[0]):
        return lib.grafp_self_match_f32(p0, 100, fake[1], 4, fake[2], k, fake[3], 4, top, mv, mo, fake[4], ws,
                                        fake[5], fake[6], fake[7], fake[8], fake[9], fake[10], None)
    assert call(k=33) == -1 and b"k=33" in lib.grafp_last_error()
    assert call(top=65) == -1 and b"top" in lib.grafp_last_error()
    assert call(top=0) == -1 and b"top" in lib.grafp_last_error()
    assert call(mv=0) == -1 and b"min_votes" in lib.grafp_last_error()
    assert call(mo=0) == -1 and b"min_overlap" in lib.grafp_last_error()
    # below the header (5 region starts, 256 bytes) the call is refused; above it, sources that do not fit are marked
    # -2 by the kernel (tests/test_gpu_selfmatch.py)
    assert call(ws=255) == -2 and b"header" in lib.grafp_last_error()
    assert lib.grafp_self_match_f32(fake[0], 100, fake[1], 4, fake[2], 8, fake[3], 4, 8, 4, 1, None, ws_ok, fake[5],
                                    fake[6], fake[7], fake[8], fake[9], fake[10], None) == -2
    assert call(p0=None) == -1 and b"null pointer" in lib.grafp_last_error()


def test_workspace_is_exactly_what_the_launch_lays_out():
    """grafp_self_match_workspace sums the per-source regions of selfmatch.hip (8-byte units): records 3 x
    ceil(L k / min_votes), two phase 4-5 key arrays of pow2(max(64, records)), the hit keys pow2(L k) when above one
    LDS piece of 16 384 keys; plus the header of n_src + 1 int64, rounded up to 256 bytes."""
    def units(L, k, mv):
        if L <= 0:
            return 0
        n0 = L * k
        cap = -(-n0 // mv)
        p2 = 1 << max(6, (cap - 1).bit_length())
        p1 = 1 << max(6, (n0 - 1).bit_length())
        return 3 * cap + 2 * p2 + (p1 if p1 > 16384 else 0)
    head = lambda n_src: -(-(n_src + 1) * 8 // 256) * 256
    for rows, k, mv in (([303] * 3300, 32, 4), ([6100, 300, 0, 500, 40], 32, 1), ([1], 1, 1), ([0, 0], 8, 3),
                        ([512, 513, 2000], 32, 2), ([], 32, 4)):
        want = head(len(rows)) + 8 * sum(units(L, k, mv) for L in rows)
        assert ops.self_match_workspace_bytes(rows, k, mv) == want, (rows[:4], k, mv)
    # the benchmark's launch: 999 900 rows at k = 32, min_votes 4 -> 124 KB per 303-row source
    assert ops.self_match_workspace_bytes([303] * 3300, 32, 4) == 26624 + 3300 * 15464 * 8


def test_selfmatch_kernel_has_no_packed_f32_instructions():
    """The shipped object's own command (make -n), compiled to device assembly: no packed-f32 instruction in
    selfmatch.hip."""
    asm = shipped_asm("selfmatch")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert sum("self_match_kernel" in k for k in kernels) == 1
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm


# ---- host bookkeeping of the library -------------------------------------------------------------------------------
def _match(a, b, m, la, lb, score=0.99):
    return {"track_a": a, "track_b": b, "score": score, "coverage": m / min(la, lb)}


def test_duplicate_groups_on_hand_made_matches():
    ms = [_match(0, 3, 95, 100, 100), _match(3, 0, 95, 100, 100),      # 0 ~ 3
          _match(3, 7, 50, 100, 52),                                  # 3 ~ 7: covers 50 / 52 of the shorter
          _match(1, 2, 30, 100, 100),                                 # a quote: too little of either
          _match(4, 5, 100, 100, 100, score=0.3),                     # covers, but too weak
          _match(8, 9, 100, 100, 100)]
    assert library.FingerprintLibrary.duplicate_groups(ms) == [[0, 3, 7], [8, 9]]
    assert library.FingerprintLibrary.duplicate_groups(ms, min_score=None) == [[0, 3, 7], [4, 5], [8, 9]]
    assert library.FingerprintLibrary.duplicate_groups(ms, min_coverage=0.25) == [[0, 3, 7], [1, 2], [8, 9]]
    assert library.FingerprintLibrary.duplicate_groups([]) == []


def test_self_matches_coverage_and_seconds_on_a_cpu_library(monkeypatch):
    """self_matches' host side with the search and the kernel replaced by the restatement."""
    from grafp_amd.train import build_model
    from grafp_amd.util import load_config
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg)
    rows = _rows(60, 12)
    rows[30:40] = rows[5:15]                                    # track 2 (rows 30..49) starts with rows 5..14 of
    rows[30:40, 0] += 1 / 256                                   # track 0, nearly (every row stays unique)
    first = [0, 20, 30, 50, 60]
    lib = library.FingerprintLibrary(model, cfg, torch.from_numpy(rows), first, ["a", "b", "c", "d"], device="cpu")
    ids_all = np.full((60, 2), -1, np.int64)
    for i in range(10):
        ids_all[5 + i, 0], ids_all[30 + i, 0] = 30 + i, 5 + i

    class _Index:
        def search(self, q, k):
            g = [int(np.flatnonzero((rows == r).all(1))[0]) for r in q.numpy()]
            return None, torch.from_numpy(ids_all[g, :k])

    monkeypatch.setattr(library.FingerprintLibrary, "index", property(lambda self: _Index()))
    monkeypatch.setattr(ops, "self_match", lambda r, f, ids, tracks, top, min_votes, min_overlap: tuple(
        torch.from_numpy(x) for x in self_match_ref(r.numpy(), f.numpy(), ids.numpy(), tracks.tolist(), top,
                                                    min_votes, min_overlap)))
    ms = lib.self_matches(k_probe=2, min_overlap_s=0.5, batch_rows=25)
    seg = lib.segment_s
    assert [(m["track_a"], m["track_b"], m["offset"]) for m in ms] == [(0, 2, -5), (2, 0, 5)]
    m = ms[0]
    assert m["name_a"] == "a" and m["name_b"] == "c" and m["votes"] == 10
    assert m["a_start_s"] == 5 * seg and m["b_start_s"] == 0.0 and m["overlap_s"] == 10 * seg
    assert m["coverage"] == 10 / 20 and m["score"] == score_run(rows[5:15], rows[30:40])
    assert ms[1]["a_start_s"] == 0.0 and ms[1]["b_start_s"] == 5 * seg
    assert lib.self_matches(k_probe=2, min_overlap_s=0.5, tracks=[2]) == ms[1:]
    assert lib.self_matches(k_probe=2, min_overlap_s=1.1) == []            # 12 rows needed, 10 shared
    assert lib.duplicate_groups(ms, min_coverage=0.5, min_score=0.5) == [[0, 2]]
    assert lib.duplicate_groups(ms, min_score=0.5) == [] and lib.duplicate_groups(ms, min_coverage=0.5) == []


def test_command_line_parses_dedup(capsys):
    from grafp_amd import identify
    with pytest.raises(SystemExit) as e:
        identify.main(["dedup", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--min-overlap" in out and "--coverage" in out and "--json" in out and "--library" in out
    with pytest.raises(SystemExit) as e:
        identify.main(["dedup", "--library", "lib"])                 # --ckp is required
    assert e.value.code == 2
