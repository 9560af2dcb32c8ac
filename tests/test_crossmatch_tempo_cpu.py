"""CPU tests of whole recordings that play faster or slower than the catalogue (csrc/crossmatch_tempo.hip,
ops.cross_match_tempo, FingerprintLibrary.match(tempo=...)): the numpy restatement against the dense one and on hand-built
cases, the refusal paths of the op and of the C entry, the workspace formula, the ABI conventions, the shipped assembly,
the library's refusals and derived fields, and the command line.  No GPU call is made."""
import ctypes
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _crossmatch_ref import cross_match_ref
from _crossmatch_tempo_ref import cross_match_tempo_ref, cross_match_tempo_source, short_case
from _identify_ref import score_run
from _identify_tempo_ref import w
from grafp_amd import library, ops
from grafp_amd.util import load_config


def _rows(n, seed):
    """Dyadic rows (multiples of 2^-8 in [-1/8, 1/8)): every product and partial sum is exact in f32."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-32, 32, size=(n, 128)) / 256.0).astype(np.float32)


# ---- the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,min_votes,min_overlap", [(1, 1, 1), (8, 4, 1), (8, 3, 6), (32, 1, 1)])
def test_the_ratio_one_is_the_dense_restatement(k, min_votes, min_overlap):
    case = short_case(10 + k, k, [256])
    got = cross_match_tempo_ref(*case, [256], top=8, min_votes=min_votes, min_overlap=min_overlap)
    want = cross_match_ref(*case, top=8, min_votes=min_votes, min_overlap=min_overlap)
    for g, x, name in zip(got, want, ("track", "delta", "start", "length", "score", "votes")):
        assert g.dtype == x.dtype and np.array_equal(g, x), name
    assert (got[0][:, 0] >= 0).sum() >= 20
    assert np.array_equal(got[6], np.where(got[0] >= 0, 256, 0))


def test_a_slow_source_reads_one_library_row_twice():
    rows = _rows(12, 1)
    first = np.array([0, 12])
    i = np.arange(2, 10)                                                      # the source's rows 0 and 1 hit nothing
    assert w(i, 128).tolist() == [1, 2, 2, 3, 3, 4, 4, 5]                     # counted from the source's row 0
    ids = np.full((10, 1), -1)
    ids[2:, 0] = 2 + w(i, 128)                                                # a = 2: rows 3 4 4 5 5 6 6 7
    q = _rows(10, 9)
    q[2:] = rows[ids[2:, 0]]
    res = cross_match_tempo_source(rows, first, q, ids, [128, 256], min_votes=4)
    assert [(b, d, lo, m, v, num) for b, d, lo, m, _, v, num in res] == [(0, 2, 2, 8, 8, 128)]
    assert res[0][4] == score_run(q[2:], rows[[3, 4, 4, 5, 5, 6, 6, 7]])
    # the dense diagonals of the same hits hold at most two of the eight rows each
    dense = cross_match_tempo_source(rows, first, q, ids, [256], min_votes=1)
    assert dense and max(r[5] for r in dense) <= 2 and max(r[3] for r in dense) <= 2


def test_a_fast_source_skips_library_rows():
    rows = _rows(14, 2)
    first = np.array([0, 14])
    at = w(np.arange(6), 512)                                                 # 0 2 4 6 8 10
    q = rows[1 + at].copy()
    res = cross_match_tempo_source(rows, first, q, (1 + at)[:, None], [256, 512], min_votes=4)
    assert [(b, d, lo, m, v, num) for b, d, lo, m, _, v, num in res] == [(0, 1, 0, 6, 6, 512)]
    assert res[0][4] == score_run(q, rows[[1, 3, 5, 7, 9, 11]])


def test_a_run_is_cut_where_it_crosses_into_the_next_track():
    rows = _rows(16, 3)
    first = np.array([0, 6, 16])                                              # tracks of 6 and 10 rows
    num = 384                                                                 # rho = 1.5: w = 0 2 3 5 6 8 9 11
    at = w(np.arange(8), num)
    assert at.tolist() == [0, 2, 3, 5, 6, 8, 9, 11]
    q = rows[1 + at].copy()
    ids = (1 + at)[:, None]                                                   # rows 1 3 4 | 6 7 9 10 12, one alignment
    res = cross_match_tempo_source(rows, first, q, ids, [num], min_votes=1)
    got = {(b, d, lo, m, v) for b, d, lo, m, _, v, _ in res}
    assert got == {(0, 1, 0, 3, 3), (1, -5, 3, 5, 5)}                         # delta = a - first[b], a = 1
    by_track = {r[0]: r for r in res}
    assert by_track[0][4] == score_run(q[:3], rows[[1, 3, 4]])
    assert by_track[1][4] == score_run(q[3:], rows[[6, 7, 9, 10, 12]])
    # the votes and the span decide, not the pairs a track could hold: 3 votes over 3 rows fail min_votes = 4
    assert [r[0] for r in cross_match_tempo_source(rows, first, q, ids, [num], min_votes=4)] == [1]
    assert cross_match_tempo_source(rows, first, q, ids, [num], min_votes=1, min_overlap=6) == []


def test_equal_scores_go_to_the_ratio_nearer_one_then_the_smaller_ratio_then_the_smaller_alignment():
    base = _rows(1, 4)
    rows = np.repeat(base, 12, axis=0)                                        # identical library rows
    first = np.array([0, 12])
    q = np.repeat(base, 4, axis=0)
    ids = np.array([[4], [5], [6], [7]])                                      # one alignment at every ratio near 1
    for ratios, want in (([200, 256, 300], 256), ([240, 272], 240), ([250, 270], 250), ([230, 262], 262)):
        res = cross_match_tempo_source(rows, first, q, ids, ratios, top=3)
        assert len(res) == 1 and res[0][6] == want, (ratios, res)
        assert res[0][4] == score_run(q, rows[:4]) and res[0][1:4] == (4, 0, 4)
    # inside one ratio the smaller alignment
    res = cross_match_tempo_source(rows, first, q, np.array([[4, 2], [5, 3], [6, 4], [7, 5]]), [256], top=3)
    assert [(b, d, v) for b, d, _, _, _, v, _ in res] == [(0, 2, 4)]
    # both alignments exist at both ratios (w is the same over four rows): the ratio decides first, then the alignment
    ids2 = np.array([[4, 2], [5, 3], [6, 4], [7, 5]])
    res = cross_match_tempo_source(rows, first, q, ids2, [240, 256], top=3)
    assert [(b, d, num) for b, d, _, _, _, _, num in res] == [(0, 2, 256)]


def test_many_ratios_win_on_the_short_case():
    ratios = [243, 256, 269]
    case = short_case(18, 8, ratios)
    got = cross_match_tempo_ref(*case, ratios, top=8, min_votes=4, min_overlap=1)
    found = got[0][:, 0] >= 0
    assert found.sum() >= 20 and set(np.unique(got[6][got[0] >= 0]).tolist()) == set(ratios)
    for s in (0, 7, 59):
        assert (got[0][s] == -1).all() and (got[6][s] == 0).all() and np.isneginf(got[4][s]).all()


# ---- the op ---------------------------------------------------------------------------------------------------------
def test_cross_match_tempo_op_refusals_without_a_gpu():
    rows = torch.zeros(8, 128)
    q = torch.zeros(30, 128)
    first = torch.tensor([0, 8])
    src = torch.tensor([0, 10, 30])
    ids = torch.zeros(30, 4, dtype=torch.int64)
    r = [250, 256]
    with pytest.raises(ValueError, match="top"):
        ops.cross_match_tempo(rows, first, q, src, ids, r, top=65)
    with pytest.raises(ValueError, match="k=33"):
        ops.cross_match_tempo(rows, first, q, src, torch.zeros(30, 33, dtype=torch.int64), r)
    with pytest.raises(ValueError, match="min_votes"):
        ops.cross_match_tempo(rows, first, q, src, ids, r, min_votes=0)
    with pytest.raises(ValueError, match="min_overlap"):
        ops.cross_match_tempo(rows, first, q, src, ids, r, min_overlap=0)
    with pytest.raises(ValueError, match="never decrease"):
        ops.cross_match_tempo(rows, torch.tensor([0, 5, 3, 8]), q, src, ids, r)
    with pytest.raises(ValueError, match="source table"):
        ops.cross_match_tempo(rows, first, q, torch.tensor([0, 20, 10, 30]), ids, r)
    with pytest.raises(ValueError, match="source table"):
        ops.cross_match_tempo(rows, first, q, torch.tensor([0, 29]), ids, r)
    with pytest.raises(ValueError, match="topk_ids"):
        ops.cross_match_tempo(rows, first, q, src, ids[:29], r)
    with pytest.raises(ValueError, match="0 ratios"):
        ops.cross_match_tempo(rows, first, q, src, ids, [])
    with pytest.raises(ValueError, match="65 ratios"):
        ops.cross_match_tempo(rows, first, q, src, ids, list(range(200, 265)))
    for bad in ([256, 256], [260, 250]):
        with pytest.raises(ValueError, match="strictly ascending"):
            ops.cross_match_tempo(rows, first, q, src, ids, bad)
    for bad in ([127, 256], [256, 513]):
        with pytest.raises(ValueError, match=r"\[128, 512\]"):
            ops.cross_match_tempo(rows, first, q, src, ids, bad)
    # cross_match's host checks come before the ratio checks
    with pytest.raises(ValueError, match="top"):
        ops.cross_match_tempo(rows, first, q, src, ids, [], top=0)
    # a source of more than 4 194 303 rows (only shapes are read before the refusal: no such arrays exist)
    assert ops.CROSS_MATCH_TEMPO_MAX_ROWS == 4194303 == (2 ** 31 - 128) // 512
    nq = ops.CROSS_MATCH_TEMPO_MAX_ROWS + 1
    with pytest.raises(ValueError, match="4194303"):
        ops.cross_match_tempo(rows, first, torch.empty((nq, 128), device="meta"), torch.tensor([0, nq]),
                              torch.empty((nq, 4), dtype=torch.int64, device="meta"), r)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.cross_match_tempo(rows, first, q, src, ids, r)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.cross_match_tempo(rows, first, q, src, ids, np.array([256], np.int32))


# ---- the C ABI entry and the shipped object -------------------------------------------------------------------------
NEW_ARGS = ["const int32_t *ratio_num", "int n_ratios", "int32_t *out_ratio"]


def test_abi_entry_follows_the_conventions():
    from test_abi import _ctype_of, _declared
    from grafp_amd import _lib
    d = _declared()
    ret, args = d["grafp_cross_match_tempo_f32"]
    assert ret == "int" and args[-1].startswith("grafp_stream_t")
    dense = d["grafp_cross_match_f32"][1]
    assert [a for a in args if a not in NEW_ARGS] == dense and all(a in args for a in NEW_ARGS)
    assert args.index("const int32_t *ratio_num") == dense.index("int min_overlap") + 1
    assert args.index("int n_ratios") == dense.index("int min_overlap") + 2
    assert args[-2] == "int32_t *out_ratio"
    res, argtypes = _lib.SIGNATURES["grafp_cross_match_tempo_f32"]
    assert res is ctypes.c_int and [_ctype_of(a) for a in args] == list(argtypes)
    assert d["grafp_cross_match_tempo_workspace"] == (
        "size_t", d["grafp_self_match_workspace"][1] + ["int n_ratios", "int top"])
    res, argtypes = _lib.SIGNATURES["grafp_cross_match_tempo_workspace"]
    assert res is ctypes.c_size_t and len(argtypes) == 6
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "grafp_cross_match_tempo_f32") and hasattr(raw, "grafp_cross_match_tempo_workspace")


@pytest.mark.parametrize("lens,k,min_votes,R,top", [([303] * 5, 32, 4, 31, 8), ([1100, 520, 40, 0], 32, 1, 2, 64),
                                                    ([37500], 20, 4, 15, 8)])
def test_workspace_is_one_header_the_regions_per_ratio_and_the_lists(lens, k, min_votes, R, top):
    dense = ops.self_match_workspace_bytes(lens, k, min_votes)
    head = ((len(lens) + 1) * 8 + 255) // 256 * 256
    want = head + R * (dense - head) + 24 * len(lens) * R * top
    assert ops.cross_match_tempo_workspace_bytes(lens, k, min_votes, R, top) == want
    assert dense > head or not any(lens)


def test_workspace_is_zero_for_arguments_out_of_range():
    from grafp_amd._lib import lib
    lens = np.array([40, 50], np.int64)
    p = ctypes.c_void_p(lens.ctypes.data)
    assert lib.grafp_cross_match_tempo_workspace(p, 2, 8, 4, 3, 8) > 0
    for R, top in ((0, 8), (65, 8), (3, 0), (3, 65)):
        assert lib.grafp_cross_match_tempo_workspace(p, 2, 8, 4, R, top) == 0
    assert lib.grafp_cross_match_tempo_workspace(p, 2, 0, 4, 3, 8) == 0       # the sibling's zeros carry over
    assert lib.grafp_cross_match_tempo_workspace(p, 2, 8, 0, 3, 8) == 0
    assert lib.grafp_cross_match_tempo_workspace(None, 2, 8, 4, 3, 8) == 0
    assert lib.grafp_cross_match_tempo_workspace(None, 0, 8, 4, 3, 8) == 256   # no source: the header alone


def test_abi_entry_refuses_out_of_range_launches_without_a_gpu():
    from grafp_amd._lib import lib
    # never dereferenced: every call below fails an argument check before anything is launched (no call here may pass
    # them -- this file also runs on machines with a GPU).  The ratios are host memory and are read.
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(14)]

    def call(k=4, top=8, min_votes=4, min_overlap=1, n=100, n_q=1000, n_src=4, ratios=(250, 256), n_ratios=None,
             rows=fake[0], ws=fake[5], ws_bytes=1 << 20, out_ratio=fake[12], nums=True):
        arr = (ctypes.c_int32 * max(1, len(ratios)))(*ratios)
        return lib.grafp_cross_match_tempo_f32(rows, n, fake[1], 2, fake[2], n_q, fake[3], n_src, fake[4], k, top,
                                               min_votes, min_overlap, ctypes.cast(arr, ctypes.c_void_p) if nums else None,
                                               len(ratios) if n_ratios is None else n_ratios, ws, ws_bytes, fake[6],
                                               fake[7], fake[8], fake[9], fake[10], fake[11], out_ratio, None)
    assert call(k=33) == -1 and b"exceeds" in lib.grafp_last_error()
    assert call(top=65) == -1 and b"top" in lib.grafp_last_error()
    assert call(top=0) == -1 and b"top" in lib.grafp_last_error()
    assert call(min_votes=0) == -1 and b"min_votes" in lib.grafp_last_error()
    assert call(min_overlap=0) == -1 and b"min_overlap" in lib.grafp_last_error()
    assert call(n_ratios=0) == -1 and b"n_ratios" in lib.grafp_last_error()
    assert call(n_ratios=65) == -1 and b"n_ratios" in lib.grafp_last_error()
    assert call(ratios=(127, 256)) == -1 and b"[128, 512]" in lib.grafp_last_error()
    assert call(ratios=(256, 513)) == -1 and b"[128, 512]" in lib.grafp_last_error()
    assert call(ratios=(256, 256)) == -1 and b"ascending" in lib.grafp_last_error()
    assert call(ratios=(260, 250)) == -1 and b"ascending" in lib.grafp_last_error()
    assert call(rows=None) == -1 and b"null pointer" in lib.grafp_last_error()
    assert call(nums=False) == -1 and b"null pointer" in lib.grafp_last_error()
    assert call(out_ratio=None) == -1 and b"null pointer" in lib.grafp_last_error()
    assert call(n=0) == -1 and b"bad sizes" in lib.grafp_last_error()
    assert call(n_q=0x7fffff00) == -1 and b"bad sizes" in lib.grafp_last_error()
    assert call(rows=ctypes.c_void_p(260)) == -1 and b"aligned" in lib.grafp_last_error()
    # the workspace: missing, below the header, below the header and the lists (4 sources x 2 ratios x top 8 x 24 bytes)
    ws_err = call(ws=None)
    assert ws_err == -2 and b"workspace" in lib.grafp_last_error()
    assert call(ws_bytes=255) == ws_err and b"workspace" in lib.grafp_last_error()
    assert call(ws_bytes=256 + 24 * 4 * 2 * 8 - 1) == ws_err and b"lists" in lib.grafp_last_error()


def test_cross_match_tempo_kernels_have_no_packed_f32_instructions():
    """The shipped object's own command (make -n), compiled to device assembly: the plan, pass 1 and the merge of pass 2
    are there, nothing else, and none holds a packed-f32 instruction."""
    asm = shipped_asm("crossmatch_tempo")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert sum("cross_match_tempo_plan_kernel" in k for k in kernels) == 1
    assert sum("cross_match_tempo_kernel" in k for k in kernels) == 1
    assert sum("cross_match_tempo_merge_kernel" in k for k in kernels) == 1 and len(kernels) == 3
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm


# ---- the library ------------------------------------------------------------------------------------------------------
def _model():
    from grafp_amd.train import build_model
    torch.manual_seed(0)
    return build_model(load_config())


def _cpu_lib(model):
    return library.FingerprintLibrary(model, load_config(), torch.from_numpy(_rows(1014, 13)), [0, 0, 700, 708, 1014],
                                      ["a", "b", "c", "d"], precision="f32", device="cpu")


def test_a_compact_or_thinned_library_refuses_match_with_tempo():
    from test_identify_pq_cpu import _compact
    model = _model()
    wave = np.zeros(16000, np.float32)
    with pytest.raises(NotImplementedError, match="tempo"):
        _cpu_lib(model).thin(2).match(wave, tempo=0.06)
    with pytest.raises(NotImplementedError, match="tempo"):
        _compact(model)[0].match(wave, tempo=0.06)
    with pytest.raises(NotImplementedError, match="row_stride"):              # without tempo: today's refusal
        _cpu_lib(model).thin(2).match(wave)
    with pytest.raises(ValueError, match="tempo"):                           # a bad range is refused before any work
        _cpu_lib(model).match(wave, tempo=0.7)
    with pytest.raises(ValueError, match="step"):                            # 103 ratios at step 1
        _cpu_lib(model).match(wave, tempo=0.2)


def test_match_fields_from_given_kernel_outputs():
    lib = _cpu_lib(_model())
    seg_s = lib.segment_s
    dense = lib._match_entry(1, 30, 5, 600, 0.75, 580, 640)
    assert list(dense) == ["track", "name", "score", "votes", "offset", "recording_start_s", "track_start_s",
                           "overlap_s", "coverage", "recording_coverage", "track_coverage"]
    assert dense == {"track": 1, "name": "b", "score": 0.75, "votes": 580, "offset": 30, "recording_start_s": 5 * seg_s,
                     "track_start_s": 35 * seg_s, "overlap_s": 600 * seg_s, "coverage": 600 / 640,
                     "recording_coverage": 600 / 640, "track_coverage": 600 / 700}
    # at ratio 256 every dense field is today's, for the recording shorter and longer than the track
    for n_rec in (640, 900, 0):
        d, t = lib._match_entry(1, 30, 5, 600, 0.75, 580, n_rec), lib._match_entry(1, 30, 5, 600, 0.75, 580, n_rec, 256)
        assert list(t) == list(d) + ["tempo", "tempo_num", "track_overlap_s"]
        assert {k: t[k] for k in d} == d
        assert (t["tempo"], t["tempo_num"], t["track_overlap_s"]) == (1.0, 256, d["overlap_s"])
    # a fast recording: rows 5 .. 604 sit on offset + w(5) .. offset + w(604)
    num, lo, m, off = 266, 5, 600, 30
    w_lo, w_hi = int(w(lo, num)), int(w(lo + m - 1, num))
    assert (w_lo, w_hi) == (5, 628)
    t = lib._match_entry(1, off, lo, m, 0.9, 600, 640, num)
    assert t["offset"] == off and t["tempo_num"] == num and t["tempo"] == num / 256
    assert t["recording_start_s"] == lo * seg_s and t["overlap_s"] == m * seg_s
    assert t["track_start_s"] == (off + w_lo) * seg_s and t["track_overlap_s"] == (w_hi - w_lo + 1) * seg_s
    assert t["recording_coverage"] == m / 640 and t["track_coverage"] == (w_hi - w_lo + 1) / 700
    assert t["coverage"] == max(t["recording_coverage"], t["track_coverage"]) == t["recording_coverage"]
    # a slow one covers less of the track than of itself
    t = lib._match_entry(3, 0, 0, 300, 0.9, 300, 300, 243)
    assert t["track_coverage"] == (int(w(299, 243)) + 1) / 306 < t["recording_coverage"] == 1.0 == t["coverage"]


def test_match_takes_a_tempo_on_the_command_line(capsys):
    from grafp_amd import identify
    with pytest.raises(SystemExit) as e:
        identify.main(["match", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--tempo" in out and "--tempo-step" in out
    assert "match --tempo" in identify.__doc__


# ---- the span arithmetic and the entries built from it ---------------------------------------------------------------
def test_tempo_span_is_the_integer_formula():
    for lo, m in ((0, 1), (0, 7), (5, 12), (300, 1), (1234, 4321)):
        assert library.tempo_span(lo, m, 256) == (lo, m)
        for num in range(128, 385):
            w_lo, w_hi = (lo * num + 128) >> 8, ((lo + m - 1) * num + 128) >> 8
            assert library.tempo_span(lo, m, num) == (w_lo, w_hi - w_lo + 1), (lo, m, num)
            assert (w_lo, w_hi) == (int(w(lo, num)), int(w(lo + m - 1, num)))


def test_match_and_self_match_entries_are_the_ones_written_before():
    """_match_entry and _self_match_entry on the library of test_identify_tempo_cpu._cpu_lib (tracks of 0, 7, 1 and 6
    rows): the dicts are literals computed with the code as it stood before tempo_span and _self_match_entry."""
    from test_identify_tempo_cpu import _cpu_lib
    lib = _cpu_lib()
    assert lib.segment_s == 0.096
    assert lib._match_entry(3, -2, 4, 5, 0.75, 6, 9) == {
        "track": 3, "name": "d", "score": 0.75, "votes": 6, "offset": -2, "recording_start_s": 0.384,
        "track_start_s": 0.192, "overlap_s": 0.48, "coverage": 0.8333333333333334,
        "recording_coverage": 0.5555555555555556, "track_coverage": 0.8333333333333334}
    assert lib._match_entry(1, 3, 2, 6, 0.5, 7, 20, 320) == {
        "track": 1, "name": "b", "score": 0.5, "votes": 7, "offset": 3, "recording_start_s": 0.192,
        "track_start_s": 0.5760000000000001, "overlap_s": 0.5760000000000001, "coverage": 1.0,
        "recording_coverage": 0.3, "track_coverage": 1.0, "tempo": 1.25, "tempo_num": 320, "track_overlap_s": 0.672}
    assert lib._self_match_entry(1, 3, -1, 2, 4, 0.75, 5) == {
        "track_a": 1, "name_a": "b", "track_b": 3, "name_b": "d", "offset": -1, "a_start_s": 0.192,
        "b_start_s": 0.096, "overlap_s": 0.384, "coverage": 0.6666666666666666, "score": 0.75, "votes": 5}
    assert lib._self_match_entry(3, 1, 2, 1, 5, 0.5, 4, 200) == {
        "track_a": 3, "name_a": "d", "track_b": 1, "name_b": "b", "offset": 2, "a_start_s": 0.096,
        "b_start_s": 0.28800000000000003, "overlap_s": 0.48, "coverage": 0.8333333333333334, "score": 0.5, "votes": 4,
        "tempo": 0.78125, "tempo_num": 200, "b_overlap_s": 0.384}
    for entry, keys in ((lib._match_entry(1, 3, 2, 6, 0.5, 7, 20, 320), "track name score votes offset "
                         "recording_start_s track_start_s overlap_s coverage recording_coverage track_coverage tempo "
                         "tempo_num track_overlap_s"),
                        (lib._self_match_entry(3, 1, 2, 1, 5, 0.5, 4, 200), "track_a name_a track_b name_b offset "
                         "a_start_s b_start_s overlap_s coverage score votes tempo tempo_num b_overlap_s")):
        assert list(entry) == keys.split()                                     # the order the keys were written in
