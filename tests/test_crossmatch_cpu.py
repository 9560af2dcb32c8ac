"""CPU tests of matching whole recordings against a library (csrc/crossmatch.hip, ops.cross_match / cross_match_pq,
FingerprintLibrary.match): the numpy restatement on hand-built cases and against the self-match and identify
restatements, the refusal paths, the C ABI entries, the shipped assembly, the library's bookkeeping on both forms and
the command line.  No GPU call is made."""
import ctypes
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _crossmatch_ref import cross_match_pq_ref, cross_match_ref, cross_match_source
from _identify_pq_ref import decode
from _identify_ref import identify_item, score_run
from _selfmatch_ref import self_match_track
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


def _shape(res):
    return [(b, d, lo, m, v) for b, d, lo, m, _, v in res]


# ---- the restatement on hand-built cases ---------------------------------------------------------------------------
def test_a_source_equal_to_a_library_track_finds_it_at_delta_zero():
    first = np.array([0, 6, 12])
    rows = _rows(12, 1)
    q = rows[6:12].copy()
    ids = _ids(6, 2, {i: [6 + i] + [7 + i] * (i < 5) for i in range(6)})   # its own row, and the next (as at overlap 0.9)
    res = cross_match_source(rows, first, q, ids, min_votes=4)
    # nothing is dropped: delta 0 (6 votes) and delta 1 (5 votes) are both eligible, and the partner keeps its best
    assert _shape(res) == [(1, 0, 0, 6, 6)]
    assert res[0][4] == score_run(q, rows[6:12])


def test_a_negative_delta_when_the_recording_starts_before_the_track():
    first = np.array([0, 8, 20])
    rows = _rows(20, 2)
    q = _rows(10, 3)
    q[4:10] = rows[8:14]                                                 # rows 4..9 of the recording = rows 0..5 of track 1
    ids = _ids(10, 1, {4 + j: [8 + j] for j in range(6)})
    (b, d, lo, m, sc, v), = cross_match_source(rows, first, q, ids, min_votes=4)
    assert (b, d, lo, m, v) == (1, -4, 4, 6, 6)
    assert sc == score_run(q[4:10], rows[8:14])


def test_span_is_taken_from_the_min_and_max_voting_rows():
    first = np.array([0, 10, 30])
    rows = _rows(30, 4)
    q = _rows(12, 5)
    # rows 2, 5 and 7 of the recording hit track 1 at delta 4 (rows 6, 9, 11 of track 1 = global 16, 19, 21)
    ids = _ids(12, 3, {2: [16], 5: [19, -1, 3], 7: [21]})
    (b, d, lo, m, sc, v), = cross_match_source(rows, first, q, ids, min_votes=3)
    assert (b, d, lo, m, v) == (1, 4, 2, 6, 3)
    assert sc == score_run(q[2:8], rows[16:22])                          # every row of the span, voting or not
    assert cross_match_source(rows, first, q, ids, min_votes=3, min_overlap=7) == []
    assert cross_match_source(rows, first, q, ids, min_votes=4) == []


def test_score_ties_go_to_the_smaller_delta():
    base, other = _rows(3, 6), _rows(3, 7)
    first = np.array([0, 3, 12])
    rows = np.concatenate([other, other, base, base])                    # track 1 = other + base + base
    ids = _ids(3, 2, {0: [9, 6], 1: [10, 7], 2: [11, 8]})               # delta 6 listed first, delta 3 ties it
    res = cross_match_source(rows, first, base, ids, min_votes=3)
    assert [(b, d, v) for b, d, _, _, _, v in res] == [(1, 3, 3)]
    ids2 = _ids(3, 2, {0: [3, 6], 1: [4, 7], 2: [5, 8]})                # delta 0 (the other rows) scores lower
    res2 = cross_match_source(rows, first, base, ids2, min_votes=3)
    assert [(b, d) for b, d, *_ in res2] == [(1, 3)] and res2[0][4] == score_run(base, base)


def test_ordering_by_score_then_track():
    base = _rows(4, 8)
    first = np.array([0, 4, 8, 12, 16])
    rows = np.concatenate([_rows(4, 9), base * 0.5, base, base])         # tracks 2 and 3 equal the recording, 1 half
    ids = _ids(4, 3, {i: [4 + i, 8 + i, 12 + i] for i in range(4)})
    res = cross_match_source(rows, first, base, ids, min_votes=4)
    assert [b for b, *_ in res] == [2, 3, 1]
    assert res[0][4] == res[1][4] > res[2][4]
    assert [b for b, *_ in cross_match_source(rows, first, base, ids, top=2, min_votes=4)] == [2, 3]


def test_zero_row_sources_bad_ids_and_duplicate_votes():
    first = np.array([0, 0, 5, 5, 10, 10])
    rows = _rows(10, 10)
    q = _rows(3, 11)
    ids = _ids(3, 3, {0: [5, 5, -1], 1: [6, 99, -7], 2: [7, 10, -1]})    # 10 = n: out of range
    src_first = np.array([0, 0, 3, 3])                                   # sources 0 and 2 have no rows
    b_, d_, lo_, m_, sc_, v_ = cross_match_ref(rows, first, q, src_first, ids, top=3, min_votes=4)
    assert b_.tolist() == [[-1, -1, -1], [3, -1, -1], [-1, -1, -1]]
    assert (d_[1, 0], lo_[1, 0], m_[1, 0], v_[1, 0]) == (0, 0, 3, 4)     # the duplicate id votes twice
    assert d_[0, 0] == INT_MIN and lo_[0, 0] == -1 and m_[0, 0] == 0 and np.isneginf(sc_[0, 0]) and v_[0, 0] == 0
    assert cross_match_ref(rows, first, q, src_first, ids, top=3, min_votes=5)[0].max() == -1


def test_a_run_that_crosses_a_track_boundary_splits_into_two_candidates():
    first = np.array([0, 4, 9, 12])
    rows = _rows(12, 12)
    q = rows[1:8].copy()                                                 # global rows 1..7: 3 of track 0, 4 of track 1
    ids = _ids(7, 1, {i: [1 + i] for i in range(7)})
    res = cross_match_source(rows, first, q, ids, min_votes=1)
    assert sorted(_shape(res)) == [(0, 1, 0, 3, 3), (1, -3, 3, 4, 4)]
    assert cross_match_source(rows, first, q, ids, min_votes=4)[0][:4] == (1, -3, 3, 4)
    got = {b: sc for b, _, _, _, sc, _ in res}
    assert got[0] == score_run(q[:3], rows[1:4]) and got[1] == score_run(q[3:], rows[4:8])


# ---- the restatements against each other ---------------------------------------------------------------------------
def test_a_library_track_as_the_source_equals_self_match():
    rng = np.random.RandomState(13)
    first = np.array([0, 7, 7, 20, 31, 40])
    rows = _rows(40, 14)
    rows[31:38] = rows[0:7]
    ids = rng.randint(-2, 41, size=(40, 4)).astype(np.int64)
    ids[:7, 0] = np.arange(31, 38)
    ids[20:31, 1] = np.arange(3, 14)
    for a in (0, 1, 2, 3, 4):
        fa, fb = int(first[a]), int(first[a + 1])
        own = ids[fa:fb].copy()
        own[(own >= fa) & (own < fb)] = -1                               # the hits self-match drops
        for mv, mo in ((1, 1), (2, 3)):
            assert cross_match_source(rows, first, rows[fa:fb], own, min_votes=mv, min_overlap=mo) == \
                self_match_track(rows, first, ids, a, min_votes=mv, min_overlap=mo), (a, mv, mo)


def test_a_span_inside_one_track_scores_as_identify():
    first = np.array([0, 12, 30])
    rows = _rows(30, 15)
    q = _rows(5, 16)
    ids = np.arange(15, 20)[:, None]                                     # the recording on rows 3..7 of track 1
    (b, d, lo, m, sc, v), = cross_match_source(rows, first, q, ids, min_votes=5)
    (t, off, isc, iv), = identify_item(rows, first, q, ids)
    assert (t, off, iv) == (1, 3, 5) and (b, lo + d, m, v) == (1, 3, 5, 5)
    assert sc == isc                                                     # the same bits


# ---- host refusals, the ABI entries and the shipped object -----------------------------------------------------------
def _pq_args(n=8, M=16, nlist=2):
    return (torch.zeros(n, dtype=torch.int32), torch.zeros((n, M), dtype=torch.uint8), torch.zeros(nlist, 128),
            torch.zeros(M, 256, 128 // M))


def test_cross_match_op_refusals_without_a_gpu():
    rows, q = torch.zeros(8, 128), torch.zeros(6, 128)
    first, src = torch.tensor([0, 3, 8]), torch.tensor([0, 2, 6])
    ids = torch.zeros(6, 4, dtype=torch.int64)
    for call, name in ((lambda *a, **kw: ops.cross_match(rows, *a, **kw), "cross_match"),
                       (lambda *a, **kw: ops.cross_match_pq(*_pq_args(), *a, **kw), "cross_match_pq")):
        with pytest.raises(ValueError, match="k=33"):
            call(first, q, src, torch.zeros(6, 33, dtype=torch.int64))
        with pytest.raises(ValueError, match="top"):
            call(first, q, src, ids, top=65)
        with pytest.raises(ValueError, match="top"):
            call(first, q, src, ids, top=0)
        with pytest.raises(ValueError, match="at least 1"):
            call(first, q, src, ids, min_votes=0)
        with pytest.raises(ValueError, match="at least 1"):
            call(first, q, src, ids, min_overlap=0)
        with pytest.raises(ValueError, match="never decrease"):
            call(torch.tensor([0, 5, 3, 8]), q, src, ids)
        with pytest.raises(ValueError, match="source table"):
            call(first, q, torch.tensor([0, 4, 2, 6]), ids)
        with pytest.raises(ValueError, match="source table"):
            call(first, q, torch.tensor([0, 2, 5]), ids)
        with pytest.raises(ValueError, match="source table"):
            call(first, q, torch.tensor([1, 2, 6]), ids)
        with pytest.raises(ValueError, match="source rows"):
            call(first, q, src, torch.zeros(5, 4, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="no CPU"):
            call(first, q, src, ids)
    lid, codes, cent, books = _pq_args()
    tail = (first, q, src, ids)
    with pytest.raises(ValueError, match="uint8"):
        ops.cross_match_pq(lid, codes.to(torch.int32), cent, books, *tail)
    with pytest.raises(ValueError, match="M=8"):
        ops.cross_match_pq(lid, torch.zeros((8, 8), dtype=torch.uint8), cent, torch.zeros(8, 256, 16), *tail)
    with pytest.raises(ValueError, match="list_id"):
        ops.cross_match_pq(lid[:7], codes, cent, books, *tail)
    with pytest.raises(ValueError, match="centroids"):
        ops.cross_match_pq(lid, codes, torch.zeros(2, 64), books, *tail)
    with pytest.raises(ValueError, match="codebooks"):
        ops.cross_match_pq(lid, codes, cent, torch.zeros(16, 256, 4), *tail)
    with pytest.raises(ValueError, match="list id lies outside"):
        ops.cross_match_pq(lid + 2, codes, cent, books, *tail)


def test_abi_entries_follow_the_conventions():
    from test_abi import _ctype_of, _declared
    from grafp_amd import _lib
    d = _declared()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("grafp_cross_match_f32", "grafp_cross_match_pq_f32"):
        ret, args = d[name]
        res, argtypes = _lib.SIGNATURES[name]
        assert [_ctype_of(a) for a in args] == list(argtypes), name
        assert ret == "int" and res is ctypes.c_int and args[-1].startswith("grafp_stream_t"), name
        assert hasattr(raw, name), name


def test_abi_entries_refuse_out_of_range_launches_without_a_gpu():
    from grafp_amd._lib import lib
    # never dereferenced: every call below fails an argument check before anything is launched
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(16)]
    ws_ok = ops.self_match_workspace_bytes([25, 25, 25, 25], 8, 4)

    def f32(k=8, top=8, mv=4, mo=1, ws=ws_ok, p0=fake[0], wsp=fake[4], n=100, nq=100, q=fake[2]):
        return lib.grafp_cross_match_f32(p0, n, fake[1], 4, q, nq, fake[3], 4, fake[5], k, top, mv, mo, wsp, ws,
                                         fake[6], fake[7], fake[8], fake[9], fake[10], fake[11], None)

    def pq(k=8, top=8, mv=4, mo=1, ws=ws_ok, p0=fake[0], wsp=fake[4], n=100, nq=100, q=fake[2], M=64, codes=fake[12]):
        return lib.grafp_cross_match_pq_f32(p0, codes, n, fake[13], 16, fake[14], M, fake[1], 4, q, nq, fake[3], 4,
                                            fake[5], k, top, mv, mo, wsp, ws, fake[6], fake[7], fake[8], fake[9],
                                            fake[10], fake[11], None)
    for call in (f32, pq):
        assert call(k=33) == -1 and b"k=33" in lib.grafp_last_error()
        assert call(top=65) == -1 and b"top" in lib.grafp_last_error()
        assert call(top=0) == -1 and b"top" in lib.grafp_last_error()
        assert call(mv=0) == -1 and b"min_votes" in lib.grafp_last_error()
        assert call(mo=0) == -1 and b"min_overlap" in lib.grafp_last_error()
        # below the header (5 region starts, 256 bytes) the call is refused with the workspace status
        assert call(ws=255) == -2 and b"header" in lib.grafp_last_error()
        assert call(wsp=None) == -2
        assert call(p0=None) == -1 and b"null pointer" in lib.grafp_last_error()
        assert call(n=0) == -1 and b"bad sizes" in lib.grafp_last_error()
        assert call(n=2 ** 31) == -1 and b"bad sizes" in lib.grafp_last_error()
        assert call(nq=2 ** 31) == -1 and b"bad sizes" in lib.grafp_last_error()
        assert call(q=ctypes.c_void_p(264)) == -1 and b"aligned" in lib.grafp_last_error()
    assert pq(M=48) == -1 and b"M=48" in lib.grafp_last_error()
    assert pq(codes=ctypes.c_void_p(258)) == -1 and b"aligned" in lib.grafp_last_error()


def test_crossmatch_kernels_have_no_packed_f32_instructions():
    """The shipped object's own command (make -n), compiled to device assembly: one f32 kernel, the four PQ
    instantiations and no packed-f32 instruction in crossmatch.hip."""
    asm = shipped_asm("crossmatch")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert sum("cross_match_kernel" in k for k in kernels) == 1
    assert sum("cross_match_pq_kernel" in k for k in kernels) == 4
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm


# ---- host bookkeeping of the library -------------------------------------------------------------------------------
def _tiny_model():
    from grafp_amd.train import build_model
    from grafp_amd.util import load_config
    cfg = load_config()
    torch.manual_seed(0)
    return cfg, build_model(cfg)


def _patch(monkeypatch, lib_rows, rec_rows, rec_counts, ids_all):
    """The fingerprints, the search and the two ops replaced: the recordings' rows are rec_rows, a searched row finds
    the hits ids_all lists for it, the ops are the restatements."""
    class _Index:
        def search(self, q, k):
            g = [int(np.flatnonzero((rec_rows == r).all(1))[0]) for r in q.numpy()]
            return None, torch.from_numpy(ids_all[g, :k])

    calls = []

    def fingerprints(self, waves, max_segments):
        assert len(waves) == len(rec_counts)
        return torch.from_numpy(rec_rows), list(rec_counts)

    def f32(rows, first, q, src, ids, top, min_votes, min_overlap):
        calls.append(("f32", int(q.shape[0])))
        assert np.array_equal(rows.numpy(), lib_rows)
        return tuple(torch.from_numpy(x) for x in cross_match_ref(rows.numpy(), first.numpy(), q.numpy(), src.numpy(),
                                                                  ids.numpy(), top, min_votes, min_overlap))

    def pq(list_id, codes, cent, books, first, q, src, ids, top, min_votes, min_overlap):
        calls.append(("pq", int(q.shape[0])))
        return tuple(torch.from_numpy(x) for x in cross_match_pq_ref(
            list_id.numpy(), codes.numpy(), cent.numpy(), books.numpy(), first.numpy(), q.numpy(), src.numpy(),
            ids.numpy(), top, min_votes, min_overlap))

    monkeypatch.setattr(library.FingerprintLibrary, "index", property(lambda self: _Index()))
    monkeypatch.setattr(library.FingerprintLibrary, "_fingerprint_tracks", fingerprints)
    monkeypatch.setattr(ops, "cross_match", f32)
    monkeypatch.setattr(ops, "cross_match_pq", pq)
    return calls


def test_match_seconds_and_coverages_on_cpu_libraries_of_both_forms(monkeypatch):
    """match's host side on a flat and a from_codes library over the same (decoded) rows."""
    cfg, model = _tiny_model()
    rng = np.random.RandomState(17)
    M, nlist, n = 16, 4, 60
    quant = {"centroids": torch.from_numpy((rng.randint(-16, 16, size=(nlist, 128)) / 256.0).astype(np.float32)),
             "codebooks": torch.from_numpy((rng.randint(-16, 16, size=(M, 256, 8)) / 256.0).astype(np.float32))}
    list_id = rng.randint(0, nlist, size=n).astype(np.int32)
    codes = rng.randint(0, 256, size=(n, M)).astype(np.uint8)
    rows = decode(list_id, codes, quant["centroids"].numpy(), quant["codebooks"].numpy())
    first = [0, 20, 30, 50, 60]
    names = ["a", "b", "c", "d"]
    # recording 0 (25 rows): rows 3..14 are rows 5..16 of track "a" (12 rows), rows 15..24 all of track "b";
    # recording 1: no rows; recording 2 (8 rows): the first 8 rows of track "c"; recording 3 (6 rows): nothing
    rec = (rng.randint(-32, 32, size=(39, 128)) / 256.0).astype(np.float32)
    rec[3:15], rec[15:25], rec[25:33] = rows[5:17], rows[20:30], rows[30:38]
    assert len({r.tobytes() for r in rec}) == 39                          # the fake index finds a row by its values
    counts = [25, 0, 8, 6]
    ids_all = np.full((39, 2), -1, np.int64)
    ids_all[3:15, 0], ids_all[15:25, 0], ids_all[25:33, 1] = np.arange(5, 17), np.arange(20, 30), np.arange(30, 38)
    waves = [np.zeros(4, np.float32)] * 4
    flat = library.FingerprintLibrary(model, cfg, torch.from_numpy(rows), first, names, device="cpu")
    comp = library.FingerprintLibrary.from_codes(model, cfg, quant, torch.from_numpy(list_id), torch.from_numpy(codes),
                                                 first, names, device="cpu")
    calls = _patch(monkeypatch, rows, rec, counts, ids_all)
    seg = flat.segment_s
    res = flat.match(waves, k_probe=2, min_overlap_s=0.5)
    assert calls == [("f32", 39)]
    assert [sorted((m["track"], m["offset"]) for m in r) for r in res] == [[(0, 2), (1, -15)], [], [(2, 0)], []]
    by = {m["track"]: m for m in res[0]}
    a, b, c = by[0], by[1], res[2][0]
    assert a["name"] == "a" and a["votes"] == 12 and a["score"] == score_run(rec[3:15], rows[5:17])
    assert a["recording_start_s"] == 3 * seg and a["track_start_s"] == 5 * seg and a["overlap_s"] == 12 * seg
    assert a["coverage"] == 12 / 20 and a["recording_coverage"] == 12 / 25 and a["track_coverage"] == 12 / 20
    assert b["recording_start_s"] == 15 * seg and b["track_start_s"] == 0.0 and b["overlap_s"] == 10 * seg
    assert b["coverage"] == 1.0 and b["recording_coverage"] == 10 / 25 and b["track_coverage"] == 1.0
    assert c["coverage"] == 1.0 and c["recording_coverage"] == 1.0 and c["track_coverage"] == 8 / 20
    assert [m["score"] for m in res[0]] == sorted((m["score"] for m in res[0]), reverse=True)
    assert set(a) == {"track", "name", "score", "votes", "offset", "recording_start_s", "track_start_s", "overlap_s",
                      "coverage", "recording_coverage", "track_coverage"}
    # the compact library: the same answer through the PQ op; small launches give the same lists
    del calls[:]
    assert comp.match(waves, k_probe=2, min_overlap_s=0.5) == res
    assert calls == [("pq", 39)]
    del calls[:]
    assert flat.match(waves, k_probe=2, min_overlap_s=0.5, batch_rows=20) == res
    assert calls == [("f32", 25), ("f32", 14)]
    # the filters
    assert flat.match(waves, k_probe=2, min_overlap_s=1.1) == [[a], [], [], []]           # 12 rows needed
    assert flat.match(waves, k_probe=2, min_overlap_s=0.5, min_votes=11)[0] == [a]
    lo, hi = sorted((a["score"], b["score"]))
    if lo < hi:
        kept = flat.match(waves, k_probe=2, min_overlap_s=0.5, min_score=(lo + hi) / 2)[0]
        assert [m["score"] for m in kept] == [hi]
    assert flat.match(waves, k_probe=2, min_overlap_s=0.5, top=1)[0] == res[0][:1]


def test_match_single_and_list_forms_agree_and_an_empty_library_gives_nothing(monkeypatch):
    cfg, model = _tiny_model()
    rows = _rows(30, 18)
    rec = rows[10:22].copy()
    rec[:, 1] += 1 / 256
    ids_all = np.arange(10, 22)[:, None].astype(np.int64)
    lib = library.FingerprintLibrary(model, cfg, torch.from_numpy(rows), [0, 10, 30], ["x", "y"], device="cpu")
    _patch(monkeypatch, rows, rec, [12], ids_all)
    wave = np.zeros(4, np.float32)
    one = lib.match(wave, k_probe=1, min_overlap_s=0.5)
    assert isinstance(one, list) and one and isinstance(one[0], dict)
    assert lib.match([wave], k_probe=1, min_overlap_s=0.5) == [one]
    assert one[0]["track"] == 1 and one[0]["offset"] == 0 and one[0]["track_coverage"] == 12 / 20
    empty = library.FingerprintLibrary(model, cfg, None, None, device="cpu")
    assert empty.match(wave) == [] and empty.match([wave, wave]) == [[], []]


def test_command_line_parses_match(capsys):
    from grafp_amd import identify
    with pytest.raises(SystemExit) as e:
        identify.main(["match", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--min-overlap", "--min-votes", "--min-score", "--top", "--k-probe", "--json", "--library", "--force"):
        assert flag in out, flag
    with pytest.raises(SystemExit) as e:
        identify.main(["match", "--library", "lib", "a.wav"])              # --ckp is required
    assert e.value.code == 2


# ---- the batching rule of match and self_matches ---------------------------------------------------------------------
def _batches_as_self_matches_wrote_them(counts, limit):
    """self_matches' loop before library.batch_ranges: accumulate, close once at least `limit` rows are held."""
    batches, cur, cur_rows = [], [], 0
    for t in range(len(counts)):
        cur.append(t)
        cur_rows += int(counts[t])
        if cur_rows >= limit:
            batches.append(cur)
            cur, cur_rows = [], 0
    if cur:
        batches.append(cur)
    return [(b[0], b[-1] + 1) for b in batches]


def _batches_as_match_rows_wrote_them(counts, limit):
    """_match_rows' loop before library.batch_ranges: two pointers over the running sums."""
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out, s0 = [], 0
    while s0 < len(counts):
        s1 = s0 + 1
        while s1 < len(counts) and starts[s1] - starts[s0] < limit:
            s1 += 1
        out.append((s0, s1))
        s0 = s1
    return out


def test_batch_ranges_on_small_cases():
    assert library.batch_ranges([3, 0, 5, 2], 5) == [(0, 3), (3, 4)]
    assert library.batch_ranges([3, 0, 5, 2], 0) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert library.batch_ranges([3, 0, 5, 2], -7) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert library.batch_ranges([3, 0, 5, 2], 10 ** 9) == [(0, 4)]
    assert library.batch_ranges([3, 0, 5, 2], 8) == [(0, 3), (3, 4)]      # a sum that lands exactly on the limit closes
    assert library.batch_ranges([0, 0], 1) == [(0, 2)]
    assert library.batch_ranges([], 5) == [] and library.batch_ranges(np.zeros(0, np.int64), 0) == []


def test_batch_ranges_is_both_loops_it_replaces():
    rng = np.random.RandomState(5)
    for case in range(200):
        n = int(rng.randint(0, 13))
        counts = rng.randint(0, 9, size=n) * (rng.rand(n) < 0.7)             # zeros included
        sums = np.cumsum(counts)
        limit = int(rng.choice([0, -3, 1, 10 ** 9, int(rng.randint(1, 40))] + ([int(rng.choice(sums))] if n else [])))
        got = library.batch_ranges(counts, limit)
        assert got == _batches_as_self_matches_wrote_them(counts, limit), (case, counts, limit)
        assert got == _batches_as_match_rows_wrote_them(counts, limit), (case, counts, limit)
        assert library.batch_ranges(list(counts), limit) == got
