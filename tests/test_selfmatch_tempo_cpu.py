"""CPU tests of tracks that share audio at another speed inside a library (csrc/selfmatch_tempo.hip, ops.self_match_tempo,
FingerprintLibrary.self_matches(tempo=...)): the numpy restatement against the dense one and on hand-built cases, the
refusal paths of the op and of the C entry, the ABI conventions, the shipped object's build command, the library's
refusals and derived fields, and the command line.  No GPU call is made."""
import ctypes
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _identify_ref import score_run
from _identify_tempo_ref import w
from _selfmatch_ref import self_match_ref
from _selfmatch_tempo_ref import REPEATING, as_cross_match, library_case, self_match_tempo_ref, short_case
from grafp_amd import library, ops
from grafp_amd.ops import self_match_tempo          # the op this file is about: without it nothing here can run
from grafp_amd.util import load_config

NAMES = ("track", "delta", "start", "length", "score", "votes", "ratio")


def _rows(n, seed):
    """Dyadic rows (multiples of 2^-8 in [-1/8, 1/8)): every product and partial sum is exact in f32."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-32, 32, size=(n, 128)) / 256.0).astype(np.float32)


# ---- the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,min_votes,min_overlap", [(8, 4, 1), (8, 3, 6), (32, 1, 1)])
def test_the_ratio_one_is_the_dense_restatement(k, min_votes, min_overlap):
    case = short_case(10 + k, k, [256])
    sub = [41, 3, 6, 0, 5, 17]
    for tracks in (None, sub):
        got = self_match_tempo_ref(*case, [256], tracks=tracks, top=8, min_votes=min_votes, min_overlap=min_overlap)
        want = self_match_ref(*case, tracks=tracks, top=8, min_votes=min_votes, min_overlap=min_overlap)
        for g, x, name in zip(got, want, NAMES):
            assert g.dtype == x.dtype and np.array_equal(g, x), (name, tracks)
        assert np.array_equal(got[6], np.where(got[0] >= 0, 256, 0))
    full = self_match_tempo_ref(*case, [256], top=8, min_votes=min_votes, min_overlap=min_overlap)
    assert (full[0][:, 0] >= 0).sum() >= 15
    for g, f in zip(got, full):                                                 # a subset is the rows of the full result
        assert np.array_equal(g, f[sub])


def test_a_track_that_repeats_itself_yields_nothing_on_itself():
    # alone with one other track it hits nothing else: padding, at every ratio
    rows, first, ids = library_case(5, [40, 12], 4, [], p_random=0.0, repeats=[0])
    own = (ids[:40] >= 0) & (ids[:40] < 40)
    assert own.sum() >= 36 and not ((ids[:40] >= 40) & (ids[:40] < 52)).any()  # (a few are struck out as out of range)
    res = self_match_tempo_ref(rows, first, ids, [243, 256, 269], min_votes=1)
    assert (res[0] == -1).all() and (res[6] == 0).all() and np.isneginf(res[4]).all()
    # the cross-match form with the own-track hits kept does find the track on itself: the mask is what drops it
    q, src_first, hit = as_cross_match(rows, first, ids, [0], mask=False)
    from _crossmatch_tempo_ref import cross_match_tempo_ref
    kept = cross_match_tempo_ref(rows, first, q, src_first, hit, [243, 256, 269], min_votes=1)
    assert kept[0][0, 0] == 0 and kept[3][0, 0] >= 1
    # among many tracks it finds others, never itself
    for ratios in ([256], [243, 256, 269]):
        case = short_case(31, 8, ratios)
        res = self_match_tempo_ref(*case, ratios, top=64, min_votes=1)
        assert (res[0] != np.arange(60)[:, None]).all()
        assert (res[0][REPEATING] >= 0).any()


def test_equal_scores_go_to_the_ratio_nearer_one_then_the_smaller_ratio_then_the_smaller_alignment():
    base = _rows(1, 4)
    rows = np.repeat(base, 16, axis=0)                                        # identical library rows
    first = np.array([0, 12, 16])                                             # the source is track 1, rows 12..15

    def run(hits, ratios):
        ids = np.full((16, hits.shape[1]), -1, np.int64)
        ids[12:] = hits
        res = self_match_tempo_ref(rows, first, ids, ratios, tracks=[1], top=3)
        return [tuple(int(x[0, j]) for x in (res[0], res[1], res[2], res[3], res[5], res[6]))
                for j in range(3) if res[0][0, j] >= 0], res[4][0]

    one = np.array([[4], [5], [6], [7]])                                      # one alignment at every ratio near 1
    for ratios, want in (([200, 256, 300], 256), ([240, 272], 240), ([250, 270], 250), ([230, 262], 262)):
        got, score = run(one, ratios)
        assert got == [(0, 4, 0, 4, 4, want)], (ratios, got)
        assert score[0] == score_run(rows[:4], rows[:4])
    two = np.array([[4, 2], [5, 3], [6, 4], [7, 5]])
    assert run(two, [256])[0] == [(0, 2, 0, 4, 4, 256)]                       # inside one ratio the smaller alignment
    assert run(two, [240, 256])[0] == [(0, 2, 0, 4, 4, 256)]                  # the ratio decides first, then the alignment


def test_both_directions_of_a_planted_copy_are_found_at_inverse_ratios():
    lens = [0, 60, 70, 9]
    first = np.concatenate([[0], np.cumsum(lens)])
    case = library_case(8, lens, 4, [(2, 0, int(first[1]) + 2, 50, 269)], p_random=0.0, p_hit=1.0, p_back=1.0)
    # min_overlap = 30: a diagonal of 256 holds about 20 rows of a span at 269 (a score is a mean, so a short fragment of
    # rows with large norms may outscore the whole span: at min_overlap = 20 such a fragment is each direction's best)
    res = self_match_tempo_ref(*case, [243, 256, 269], min_votes=4, min_overlap=30)
    # track 2's rows 0..49 are track 1's rows 2 + w(i) at 269; track 1's rows find track 2 along the inverse slope
    assert (res[0][2, 0], res[1][2, 0], res[2][2, 0], res[3][2, 0], res[6][2, 0]) == (1, 2, 0, 50, 269)
    assert (res[0][1, 0], res[1][1, 0], res[2][1, 0], res[3][1, 0], res[6][1, 0]) == (2, -2, 2, 48, 243)
    frag = self_match_tempo_ref(*case, [243, 256, 269], min_votes=4, min_overlap=20)
    assert (frag[6][[1, 2], 0] == 256).all() and (frag[3][[1, 2], 0] == 20).all()
    assert (frag[4][[1, 2], 0] > res[4][[1, 2], 0]).all()
    for s in (0, 3):
        assert (res[0][s] == -1).all()


# ---- the op ---------------------------------------------------------------------------------------------------------
def test_self_match_tempo_op_refusals_without_a_gpu():
    rows = torch.zeros(8, 128)
    first = torch.tensor([0, 3, 8])
    ids = torch.zeros(8, 4, dtype=torch.int64)
    r = [250, 256]
    with pytest.raises(ValueError, match="0 ratios"):
        self_match_tempo(rows, first, ids, [])
    with pytest.raises(ValueError, match="65 ratios"):
        self_match_tempo(rows, first, ids, list(range(200, 265)))
    for bad in ([256, 256], [260, 250]):
        with pytest.raises(ValueError, match="strictly ascending"):
            self_match_tempo(rows, first, ids, bad)
    for bad in ([127, 256], [256, 513]):
        with pytest.raises(ValueError, match=r"\[128, 512\]"):
            self_match_tempo(rows, first, ids, bad)
    # R * top > 4096: 64 ratios x top = 64 are exactly the merge's 4096 slots and pass every host check; one more of
    # either is refused by its own limit first, so the product's refusal (shared with cross_match_tempo) is never reached
    with pytest.raises(RuntimeError, match="no CPU"):
        self_match_tempo(rows, first, ids, list(range(200, 264)), top=64)
    with pytest.raises(ValueError, match="65 ratios"):
        self_match_tempo(rows, first, ids, list(range(200, 265)), top=64)
    with pytest.raises(ValueError, match="top"):
        self_match_tempo(rows, first, ids, list(range(200, 264)), top=65)
    # self_match's host checks, under the new name, come before the ratio checks
    with pytest.raises(ValueError, match="self_match_tempo: k=33"):
        self_match_tempo(rows, first, torch.zeros(8, 33, dtype=torch.int64), r)
    with pytest.raises(ValueError, match="top"):
        self_match_tempo(rows, first, ids, [], top=65)
    with pytest.raises(ValueError, match="at least 1"):
        self_match_tempo(rows, first, ids, r, min_votes=0)
    with pytest.raises(ValueError, match="at least 1"):
        self_match_tempo(rows, first, ids, r, min_overlap=0)
    with pytest.raises(ValueError, match="never decrease"):
        self_match_tempo(rows, torch.tensor([0, 5, 3, 8]), ids, r)
    with pytest.raises(ValueError, match="rows for a library"):
        self_match_tempo(rows, first, torch.zeros(7, 4, dtype=torch.int64), r)
    for bad in ([2], [-1], [0, 1, 2]):
        with pytest.raises(ValueError, match="source tracks"):
            self_match_tempo(rows, first, ids, r, tracks=bad)
    # a track of more than 4 194 303 rows (only shapes are read before the refusal: no such arrays exist)
    n = ops.CROSS_MATCH_TEMPO_MAX_ROWS + 9
    big = (torch.empty((n, 128), device="meta"), torch.tensor([0, 8, n]),
           torch.empty((n, 4), dtype=torch.int64, device="meta"))
    with pytest.raises(ValueError, match="4194303"):
        self_match_tempo(*big, r)
    with pytest.raises(RuntimeError, match="no CPU"):                          # the short track of the same library passes
        self_match_tempo(*big, r, tracks=[0])
    with pytest.raises(RuntimeError, match="no CPU"):
        self_match_tempo(rows, first, ids, r)
    with pytest.raises(RuntimeError, match="no CPU"):
        self_match_tempo(rows, first, ids, np.array([256], np.int32), tracks=[1])


# ---- the C ABI entry and the shipped object -------------------------------------------------------------------------
NEW_ARGS = ["const int32_t *ratio_num", "int n_ratios", "int32_t *out_ratio"]


def test_abi_entry_follows_the_conventions():
    from test_abi import _ctype_of, _declared
    from grafp_amd import _lib
    d = _declared()
    ret, args = d["grafp_self_match_tempo_f32"]
    assert ret == "int" and args[-1].startswith("grafp_stream_t")
    dense = d["grafp_self_match_f32"][1]
    assert [a for a in args if a not in NEW_ARGS] == dense and all(a in args for a in NEW_ARGS)
    assert args.index("const int32_t *ratio_num") == dense.index("int min_overlap") + 1
    assert args.index("int n_ratios") == dense.index("int min_overlap") + 2
    assert args[-2] == "int32_t *out_ratio"
    # the new arguments sit where grafp_cross_match_tempo_f32 has them, counted from min_overlap
    cross = d["grafp_cross_match_tempo_f32"][1]
    assert args[args.index("int min_overlap"):] == cross[cross.index("int min_overlap"):]
    res, argtypes = _lib.SIGNATURES["grafp_self_match_tempo_f32"]
    assert res is ctypes.c_int and [_ctype_of(a) for a in args] == list(argtypes)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "grafp_self_match_tempo_f32")
    assert "grafp_self_match_tempo_workspace" not in d                          # grafp_cross_match_tempo_workspace serves


def test_abi_entry_refuses_out_of_range_launches_without_a_gpu():
    from grafp_amd._lib import lib
    # never dereferenced: every call below fails an argument check before anything is launched (no call here may pass
    # them -- this file also runs on machines with a GPU).  The ratios are host memory and are read.
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(12)]

    def call(k=4, top=8, min_votes=4, min_overlap=1, n=100, n_src=4, ratios=(250, 256), n_ratios=None, rows=fake[0],
             ws=fake[4], ws_bytes=1 << 20, out_ratio=fake[11], nums=True, n_tracks=4):
        arr = (ctypes.c_int32 * max(1, len(ratios)))(*ratios)
        return lib.grafp_self_match_tempo_f32(rows, n, fake[1], n_tracks, fake[2], k, fake[3], n_src, top, min_votes,
                                              min_overlap, ctypes.cast(arr, ctypes.c_void_p) if nums else None,
                                              len(ratios) if n_ratios is None else n_ratios, ws, ws_bytes, fake[5],
                                              fake[6], fake[7], fake[8], fake[9], fake[10], out_ratio, None)
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
    assert call(n=0x7fffff00) == -1 and b"bad sizes" in lib.grafp_last_error()
    assert call(n_tracks=0) == -1 and b"bad sizes" in lib.grafp_last_error()
    assert call(n_src=-1) == -1 and b"bad sizes" in lib.grafp_last_error()
    assert call(rows=ctypes.c_void_p(260)) == -1 and b"aligned" in lib.grafp_last_error()
    assert b"self_match_tempo" in lib.grafp_last_error()
    # the workspace: missing, below the header, below the header and the lists (4 sources x 2 ratios x top 8 x 24 bytes)
    ws_err = call(ws=None)
    assert ws_err == -2 and b"workspace" in lib.grafp_last_error()
    assert call(ws_bytes=255) == ws_err and b"workspace" in lib.grafp_last_error()
    assert call(ws_bytes=256 + 24 * 4 * 2 * 8 - 1) == ws_err and b"lists" in lib.grafp_last_error()


def test_the_workspace_is_cross_match_tempos_of_the_source_tracks_rows():
    lens = [303, 0, 520, 40]
    dense = ops.self_match_workspace_bytes(lens, 32, 4)
    assert ops.cross_match_tempo_workspace_bytes(lens, 32, 4, 31, 8) == 256 + 31 * (dense - 256) + 24 * 4 * 31 * 8
    assert not hasattr(ops, "self_match_tempo_workspace_bytes")


def test_self_match_tempo_object_is_built_without_packed_f32_instructions():
    """The shipped object's own command (make -n) carries the NOPK switch (shipped_asm asserts it), and the device assembly
    it gives holds the plan, pass 1 and the merge, nothing else, and no packed-f32 instruction."""
    asm = shipped_asm("selfmatch_tempo")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert sum("self_match_tempo_plan_kernel" in k for k in kernels) == 1
    assert sum("self_match_tempo_kernel" in k for k in kernels) == 1
    assert sum("self_match_tempo_merge_kernel" in k for k in kernels) == 1 and len(kernels) == 3
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm


# ---- the library ------------------------------------------------------------------------------------------------------
def _model():
    from grafp_amd.train import build_model
    torch.manual_seed(0)
    return build_model(load_config())


LIB_FIRST = [0, 0, 700, 708, 1014]                                             # tracks of 0, 700, 8 and 306 rows


def _cpu_lib(model):
    return library.FingerprintLibrary(model, load_config(), torch.from_numpy(_rows(1014, 13)), LIB_FIRST,
                                      ["a", "b", "c", "d"], precision="f32", device="cpu")


def test_a_compact_or_thinned_library_refuses_self_matches_with_tempo():
    from test_identify_pq_cpu import _compact
    model = _model()
    with pytest.raises(NotImplementedError, match="tempo"):
        _cpu_lib(model).thin(2).self_matches(tempo=0.06)
    with pytest.raises(NotImplementedError, match="tempo"):
        _compact(model)[0].self_matches(tempo=0.06)
    with pytest.raises(NotImplementedError, match="row_stride"):              # without tempo: today's refusal
        _cpu_lib(model).thin(2).self_matches()
    with pytest.raises(ValueError, match="tempo"):                           # a bad range is refused before any work
        _cpu_lib(model).self_matches(tempo=0.7)
    with pytest.raises(ValueError, match="step"):                            # 103 ratios at step 1
        _cpu_lib(model).self_matches(tempo=0.2)


class _Index:
    def search(self, q, k):
        return None, torch.full((q.shape[0], k), -1, dtype=torch.int64)


def _outs(entries, n_src, top):
    """Kernel outputs (n_src, top) holding `entries` {source slot: [(b, d, lo, m, score, votes, num)]}."""
    pad = (-1, -2 ** 31, -1, 0, -np.inf, 0, 0)
    outs = [np.full((n_src, top), pad[j], np.float32 if j == 4 else np.int32) for j in range(7)]
    for s, es in entries.items():
        for j, e in enumerate(es):
            for o, v in zip(outs, e):
                o[s, j] = v
    return tuple(torch.from_numpy(o) for o in outs)


def test_self_matches_fields_from_given_kernel_outputs(monkeypatch):
    """self_matches(tempo=...) with the search and the kernel replaced by stubs: the launches (ratios, batches of about
    batch_rows // R rows) and the fields of the entries at a ratio above 256, one below it and at 256."""
    lib = _cpu_lib(_model())
    seg = lib.segment_s
    monkeypatch.setattr(library.FingerprintLibrary, "index", property(lambda self: _Index()))
    # by source track: (b, delta, i_lo, m, score, votes, num)
    given = {3: [(1, 30, 5, 290, 0.75, 280, 266)], 1: [(3, 2, 10, 300, 0.5, 250, 243), (2, 0, 0, 8, 0.25, 8, 256)]}
    calls = []

    def tempo_stub(r, f, ids, nums, tracks, top, min_votes, min_overlap):
        calls.append((np.asarray(nums).tolist(), tracks.tolist(), tuple(ids.shape), top, min_votes, min_overlap))
        return _outs({s: given[t] for s, t in enumerate(tracks.tolist()) if t in given}, len(tracks), top)

    def dense_stub(r, f, ids, tracks, top, min_votes, min_overlap):
        calls.append((None, tracks.tolist()))
        return _outs({s: given[t] for s, t in enumerate(tracks.tolist()) if t in given}, len(tracks), top)[:6]

    monkeypatch.setattr(ops, "self_match_tempo", tempo_stub)
    monkeypatch.setattr(ops, "self_match", dense_stub)
    ms = lib.self_matches(tempo=0.06, batch_rows=31 * 700, top=4)
    # 31 ratios at step 1; batches of 21 700 // 31 = 700 rows: tracks [0, 1], then [2, 3]
    mo = int(np.ceil(3.0 / seg - 1e-9))
    assert calls == [(list(range(241, 272)), [0, 1], (1014, 32), 4, 4, mo), (list(range(241, 272)), [2, 3], (1014, 32), 4, 4, mo)]
    assert [(m["track_a"], m["track_b"]) for m in ms] == [(1, 3), (1, 2), (3, 1)]
    assert all(list(m) == ["track_a", "name_a", "track_b", "name_b", "offset", "a_start_s", "b_start_s", "overlap_s",
                           "coverage", "score", "votes", "tempo", "tempo_num", "b_overlap_s"] for m in ms)
    slow, same, fast = ms
    # above 256: track 3's rows 5 .. 294 sit on rows 30 + w(5) .. 30 + w(294) of track 1
    w_lo, w_hi = int(w(5, 266)), int(w(294, 266))
    assert (w_lo, w_hi) == (5, 305)
    assert (fast["offset"], fast["tempo_num"], fast["tempo"], fast["votes"], fast["score"]) == (30, 266, 266 / 256, 280, 0.75)
    assert fast["a_start_s"] == 5 * seg and fast["overlap_s"] == 290 * seg
    assert fast["b_start_s"] == (30 + w_lo) * seg and fast["b_overlap_s"] == (w_hi - w_lo + 1) * seg
    assert fast["coverage"] == max(290 / 306, 301 / 700) == 290 / 306
    assert (fast["name_a"], fast["name_b"]) == ("d", "b")
    # below 256: track 1's rows 10 .. 309 cover 285 of track 3's 306 rows, more of it than of track 1
    w_lo, w_hi = int(w(10, 243)), int(w(309, 243))
    assert (w_lo, w_hi) == (9, 293)
    assert slow["b_start_s"] == (2 + w_lo) * seg and slow["b_overlap_s"] == 285 * seg and slow["overlap_s"] == 300 * seg
    assert slow["coverage"] == max(300 / 700, 285 / 306) == 285 / 306 and slow["tempo"] == 243 / 256
    # at 256 every field is today's
    calls.clear()
    dense = lib.self_matches(batch_rows=31 * 700, top=4)
    assert calls == [(None, [0, 1, 2, 3])]                                       # (no division of batch_rows without tempo)
    assert all("tempo" not in m and len(m) == 11 for m in dense)
    assert {k: same[k] for k in dense[1]} == dense[1]
    assert (same["tempo"], same["tempo_num"], same["b_overlap_s"]) == (1.0, 256, same["overlap_s"])
    assert same["coverage"] == 8 / 8 and same["b_start_s"] == 0.0
    # min_score and tracks= act as without tempo
    calls.clear()
    assert lib.self_matches(tempo=(0.98, 1.05), tempo_step=4, tracks=[3], min_score=0.8) == []
    assert calls[0][:2] == ([252, 256, 260, 264, 268], [3])
    assert library.FingerprintLibrary.duplicate_groups(ms, min_score=0.4) == [[1, 3]]
    assert library.FingerprintLibrary.duplicate_groups(ms) == []                # DUPLICATE_MIN_SCORE stays 0.9


def test_dedup_takes_a_tempo_on_the_command_line(capsys, monkeypatch, tmp_path):
    from grafp_amd import identify
    with pytest.raises(SystemExit) as e:
        identify.main(["dedup", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--tempo" in out and "--tempo-step" in out
    assert "dedup --tempo" in identify.__doc__
    # the options reach self_matches
    seen = []

    class _Lib:
        row_stride, is_compact, names = 1, False, ["a", "b"]

        def self_matches(self, **kw):
            seen.append(kw)
            return [{"track_a": 0, "track_b": 1, "coverage": 1.0, "score": 0.95, "tempo_num": 266}]

        duplicate_groups = staticmethod(library.FingerprintLibrary.duplicate_groups)

    monkeypatch.setattr(identify, "_model", lambda cfg, ckp, device: None)
    monkeypatch.setattr(library.FingerprintLibrary, "load", staticmethod(lambda *a, **kw: _Lib()))
    assert identify.main(["dedup", "--ckp", "x", "--library", "y", "--tempo", "0.06", "--tempo-step", "2"]) == 0
    assert identify.main(["dedup", "--ckp", "x", "--library", "y"]) == 0
    assert [(kw["tempo"], kw["tempo_step"]) for kw in seen] == [(0.06, 2), (None, None)]
    out = capsys.readouterr().out
    assert '"tempo_num": 266' in out and '"group"' in out
