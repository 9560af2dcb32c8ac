"""CPU tests of identification at another speed than the catalogue's (csrc/identify_tempo.hip, ops.identify_tempo,
FingerprintLibrary.identify(tempo=...)): the numpy restatement on hand-built cases, tempo_ratios, the sloped timeline, the
refusal paths, the C ABI entry, the shipped assembly and the command line.  No GPU call is made."""
import ctypes
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _identify_ref import identify_ref, score_run
from _identify_tempo_ref import pairs_of, tempo_case, tempo_item, tempo_ref, w
from grafp_amd import library, ops
from grafp_amd.util import load_config


def _rows(n, seed):
    """Dyadic rows (multiples of 2^-8 in [-1/8, 1/8)): every product and partial sum is exact in f32."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-32, 32, size=(n, 128)) / 256.0).astype(np.float32)


# ---- the restatement ----------------------------------------------------------------------------------------------
def test_row_positions_are_integer_arithmetic():
    assert w(np.arange(5), 256).tolist() == [0, 1, 2, 3, 4]
    assert w(np.arange(8), 128).tolist() == [0, 1, 1, 2, 2, 3, 3, 4]          # (s * 128 + 128) >> 8
    assert w(np.arange(5), 512).tolist() == [0, 2, 4, 6, 8]
    assert int(w(255, 512)) == 510
    assert int(w(93, 266)) == 97 and int(w(93, 256)) == 93                    # +4 %: 3.7 rows over a 94-row query
    for num in (128, 243, 256, 257, 269, 512):                                # never decreasing, steps of at most 2
        d = np.diff(w(np.arange(256), num))
        assert d.min() >= 0 and d.max() <= 2
    # two ratios 1/256 apart differ by at most one row over the 256 rows of an item
    assert np.abs(w(np.arange(256), 257) - w(np.arange(256), 256)).max() == 1


@pytest.mark.parametrize("min_overlap", [None, 1, 3])
def test_the_ratio_one_is_the_dense_restatement(min_overlap):
    case = tempo_case(5 + (min_overlap or 0), [256], n_items=40, max_ql=24)
    got = tempo_ref(*case, [256], top=8, min_overlap=min_overlap)
    want = identify_ref(*case, top=8, min_overlap=min_overlap)
    for g, x, name in zip(got, want, ("track", "offset", "score", "votes")):
        assert np.array_equal(g, x), name
    assert (got[0][:, 0] >= 0).sum() > 20
    assert np.array_equal(got[4], np.where(got[0] >= 0, 256, 0))


def test_a_slow_recording_reads_one_library_row_twice():
    rows = _rows(10, 1)
    first = np.array([0, 10])
    s = np.arange(8)
    at = w(s, 128)                                                            # 0 1 1 2 2 3 3 4
    q = rows[2 + at].copy()
    ids = (2 + at)[:, None]
    res = tempo_item(rows, first, q, ids, [128, 256])
    assert [(t, o, v, num) for t, o, _, v, num in res] == [(0, 2, 8, 128)]
    assert pairs_of(2, 0, 10, 8, 128) == list(range(8))
    assert res[0][2] == score_run(q, rows[[2, 3, 3, 4, 4, 5, 5, 6]])
    # the dense diagonals of the same hits hold at most two of the eight rows each
    dense = tempo_item(rows, first, q, ids, [256], min_overlap=1)
    assert dense[0][3] <= 2 and dense[0][2] < res[0][2]


def test_a_fast_recording_skips_library_rows():
    rows = _rows(12, 2)
    first = np.array([0, 12])
    at = w(np.arange(5), 512)                                                 # 0 2 4 6 8
    q = rows[1 + at].copy()
    res = tempo_item(rows, first, q, (1 + at)[:, None], [256, 512])
    assert [(t, o, v, num) for t, o, _, v, num in res] == [(0, 1, 5, 512)]
    assert res[0][2] == score_run(q, rows[[1, 3, 5, 7, 9]])


def test_a_run_clipped_at_a_track_end_and_the_eligibility_cap():
    rows = _rows(16, 3)
    first = np.array([0, 6, 16])                                              # tracks of 6 and 10 rows
    num = 384                                                                 # rho = 1.5: w = 0 2 3 5 6 8 9 11
    at = w(np.arange(8), num)
    assert at.tolist() == [0, 2, 3, 5, 6, 8, 9, 11]
    q = rows[np.minimum(1 + at, 15)].copy()
    ids = (1 + at)[:, None]                                                   # rows 1 3 4 | 6 7 9 10 12
    assert pairs_of(1, 0, 6, 8, num) == [0, 1, 2] and pairs_of(1, 6, 16, 8, num) == [3, 4, 5, 6, 7]
    # need = 8; track 0 can always hold (6 * 256) // 384 = 4 pairs and the run has 3: not eligible;
    # track 1 can always hold (10 * 256) // 384 = 6 and the run has 5: not eligible either
    assert tempo_item(rows, first, q, ids, [num]) == []
    res = tempo_item(rows, first, q, ids, [num], min_overlap=5)               # need = 5: track 1 only
    assert [(t, o, v, r) for t, o, _, v, r in res] == [(1, -5, 5, num)]
    assert res[0][2] == score_run(q[3:8], rows[[6, 7, 9, 10, 12]])
    res = tempo_item(rows, first, q, ids, [num], min_overlap=3)
    assert {(t, o, v) for t, o, _, v, _ in res} == {(0, 1, 3), (1, -5, 5)}
    # a 2-row track at rho = 2: the cap is max(1, (2 * 256) // 512) = 1 pair
    first2 = np.array([0, 2, 16])
    one = tempo_item(rows, first2, rows[[1, 3, 5]].copy(), np.array([[1], [3], [5]]), [512])
    assert (0, 1, 1, 512) in {(t, o, v, r) for t, o, _, v, r in one}          # one pair satisfies min(3, 1)


def test_equal_scores_go_to_the_ratio_nearer_one_then_the_smaller_ratio():
    base = _rows(1, 4)
    rows = np.repeat(base, 12, axis=0)                                        # identical library rows
    first = np.array([0, 12])
    q = np.repeat(base, 4, axis=0)
    ids = np.array([[4], [5], [6], [7]])                                      # the diagonal of ratio 1 from row 4
    for ratios, want in (([200, 256, 300], 256), ([240, 272], 240), ([250, 270], 250), ([230, 262], 262)):
        res = tempo_item(rows, first, q, ids, ratios, top=3)
        assert len(res) == 1 and res[0][4] == want, (ratios, res)
        assert res[0][2] == score_run(q, rows[:4])
    # equal ratio preference cannot happen twice, so the smaller a only decides inside one ratio
    res = tempo_item(rows, first, q, np.array([[4, 2], [5, 3], [6, 4], [7, 5]]), [256], top=3)
    assert [(t, o, v) for t, o, _, v, _ in res] == [(0, 2, 4)]


# ---- tempo_ratios ---------------------------------------------------------------------------------------------------
def test_tempo_ratios():
    got = library.tempo_ratios(0.06, 94)
    assert got.dtype == np.int32 and got.tolist() == [256 + 2 * i for i in range(-7, 8)] and len(got) == 15
    assert library.tempo_ratios((1.02, 1.08), 94).tolist() == [262, 264, 266, 268, 270, 272, 274, 276]
    assert library.tempo_ratios((0.9, 0.95), 256).tolist() == list(range(231, 244))
    assert library.tempo_ratios((0.25, 0.52), 256, step=4).tolist() == [128, 132]          # clipped at 128
    assert library.tempo_ratios((1.98, 3.0), 256, step=2).tolist() == [508, 510, 512]      # clipped at 512
    assert library.tempo_ratios(0.5, 8).tolist() == list(range(128, 385, 32))              # g = 256 // 8
    assert library.tempo_ratios(0.06, 94, step=5).tolist() == [241, 246, 251, 256, 261, 266, 271]
    assert library.tempo_ratios(0.06, 1000).tolist() == list(range(241, 272))              # g never below 1
    with pytest.raises(ValueError, match="step"):
        library.tempo_ratios((1.001, 1.003), 8)                                             # nothing on the grid
    with pytest.raises(ValueError, match="step"):
        library.tempo_ratios(0.5, 256)                                                      # 257 ratios
    with pytest.raises(ValueError, match="tempo"):
        library.tempo_ratios(0.0, 94)
    with pytest.raises(ValueError, match="tempo"):
        library.tempo_ratios(0.6, 94)


# ---- the timeline ---------------------------------------------------------------------------------------------------
def _cpu_lib():
    from grafp_amd.train import build_model
    torch.manual_seed(0)
    model = build_model(load_config())
    return library.FingerprintLibrary(model, load_config(), torch.from_numpy(_rows(14, 13)), [0, 0, 7, 8, 14],
                                      ["a", "b", "c", "d"], precision="f32", device="cpu")


def _windows(rho, n, seg_s, tempo):
    """n windows of 3 s every second over a recording that plays track 1 from 10 s on at rho; offsets on the row grid."""
    out = []
    for i in range(n):
        u = round(i / seg_s) * seg_s                                          # the window's first segment
        off = int(round((10.0 + rho * u) / seg_s))
        m = {"track": 1, "name": "b", "offset": off, "offset_s": off * seg_s, "score": 0.9 + 0.01 * i, "votes": 30}
        if tempo:
            m.update(tempo=rho, tempo_num=int(round(rho * 256)))
        out.append({"start_s": float(i), "end_s": float(i) + 3.0, "segment_start_s": u, "matches": [m]})
    return out


def test_timeline_follows_the_slope_of_a_fast_recording():
    lib = _cpu_lib()
    seg_s = lib.segment_s
    rho = 266 / 256
    plain = lib.timeline(_windows(rho, 12, seg_s, tempo=False))
    assert len(plain) > 1                                                     # 0.04 s of drift per window splits it
    spans = lib.timeline(_windows(rho, 12, seg_s, tempo=True))
    assert len(spans) == 1
    s = spans[0]
    assert (s["start_s"], s["end_s"], s["track"], s["name"]) == (0.0, 14.0, 1, "b")
    assert abs(s["tempo"] - rho) < 1e-12 and abs(s["track_offset_s"] - 10.0) <= seg_s
    assert abs(s["score"] - np.mean([0.9 + 0.01 * i for i in range(12)])) < 1e-12
    assert "_ref" not in s and "_tempos" not in s and "_scores" not in s
    # a jump of two segment hops starts a new span, and so does another track
    jump = _windows(rho, 6, seg_s, tempo=True)
    for wd in jump[3:]:
        wd["matches"][0]["offset_s"] += 2.5 * seg_s
    assert [(s["start_s"], s["end_s"]) for s in lib.timeline(jump)] == [(0.0, 5.0), (3.0, 8.0)]


def test_timeline_without_tempo_is_unchanged():
    lib = _cpu_lib()
    seg_s = lib.segment_s
    windows = _windows(1.0, 5, seg_s, tempo=False) + _windows(1.0, 3, seg_s, tempo=False)
    windows[2]["matches"] = []
    for wd in windows[5:]:
        wd["matches"][0]["offset_s"] += 1.0                                   # another place in the track: a new span
    spans =lib.timeline(windows, min_score=0.5)
    # today's rule, restated: same track, delta within one hop, starting inside the span
    want, delta0 = [], None
    for wd in windows:
        if not wd["matches"]:
            continue
        m = wd["matches"][0]
        delta = m["offset_s"] - wd["segment_start_s"]
        if want and abs(delta - delta0) <= seg_s + 1e-9 and wd["start_s"] <= want[-1]["end_s"]:
            want[-1]["end_s"] = wd["end_s"]
            want[-1]["_s"].append(m["score"])
        else:
            want.append({"start_s": wd["start_s"], "end_s": wd["end_s"], "track": 1, "name": "b",
                         "track_offset_s": wd["start_s"] + delta, "_s": [m["score"]]})
            delta0 = delta
    for s in want:
        s["score"] = float(np.mean(s.pop("_s")))
    assert spans == want and len(spans) == 2
    assert all(list(s) == ["start_s", "end_s", "track", "name", "track_offset_s", "score"] for s in spans)


def test_a_compact_or_thinned_library_refuses_tempo():
    lib = _cpu_lib()
    with pytest.raises(NotImplementedError, match="tempo"):
        lib.thin(2).identify(np.zeros(16000, np.float32), tempo=0.06)
    with pytest.raises(NotImplementedError, match="tempo"):
        lib.thin(2).identify_windows(np.zeros(64000, np.float32), tempo=0.06)


# ---- the op ---------------------------------------------------------------------------------------------------------
def test_identify_tempo_op_refusals_without_a_gpu():
    assert ops.IDENTIFY_TEMPO_MAX_RATIOS == 64
    rows = torch.zeros(8, 128)
    q = torch.zeros(300, 128)
    first = torch.tensor([0, 8])
    ids = torch.zeros(300, 4, dtype=torch.int64)
    one = torch.zeros(1, dtype=torch.int64)
    two = torch.tensor([2], dtype=torch.int32)
    r = [250, 256]
    with pytest.raises(ValueError, match="256 segments"):
        ops.identify_tempo(rows, first, q, ids, one, torch.tensor([257], dtype=torch.int32), r)
    with pytest.raises(ValueError, match="k=33"):
        ops.identify_tempo(rows, first, q, torch.zeros(300, 33, dtype=torch.int64), one, two, r)
    with pytest.raises(ValueError, match="hits per item"):
        ops.identify_tempo(rows, first, q, torch.zeros(300, 32, dtype=torch.int64), one, two, r, max_len=257)
    with pytest.raises(ValueError, match="never decrease"):
        ops.identify_tempo(rows, torch.tensor([0, 5, 3, 8]), q, ids, one, two, r)
    with pytest.raises(ValueError, match="outside q_rows"):
        ops.identify_tempo(rows, first, q, ids, torch.tensor([299]), two, r)
    with pytest.raises(ValueError, match="top"):
        ops.identify_tempo(rows, first, q, ids, one, two, r, top=65)
    with pytest.raises(ValueError, match="min_overlap"):
        ops.identify_tempo(rows, first, q, ids, one, two, r, min_overlap=0)
    with pytest.raises(ValueError, match="0 ratios"):
        ops.identify_tempo(rows, first, q, ids, one, two, [])
    with pytest.raises(ValueError, match="65 ratios"):
        ops.identify_tempo(rows, first, q, ids, one, two, list(range(200, 265)))
    for bad in ([256, 256], [260, 250]):
        with pytest.raises(ValueError, match="strictly ascending"):
            ops.identify_tempo(rows, first, q, ids, one, two, bad)
    for bad in ([127, 256], [256, 513]):
        with pytest.raises(ValueError, match=r"\[128, 512\]"):
            ops.identify_tempo(rows, first, q, ids, one, two, bad)
    # the host checks of ops.identify come before the ratio checks
    with pytest.raises(ValueError, match="top"):
        ops.identify_tempo(rows, first, q, ids, one, two, [], top=0)
    # n + 511 must stay below 2^32 (only the row count is read before the refusal: no such array exists)
    huge = torch.empty(((1 << 32) - 511, 128), device="meta")
    with pytest.raises(ValueError, match="2\\^32"):
        ops.identify_tempo(huge, torch.tensor([0, (1 << 32) - 511]), q, ids, one, two, r)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.identify_tempo(rows, first, q, ids, one, two, r)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.identify_tempo(rows, first, q, ids, one, two, np.array([256], np.int32))


# ---- the C ABI entry and the shipped object ---------------------------------------------------------------------
NEW_ARGS = ["const int32_t *ratio_num", "int n_ratios", "void *ws", "int32_t *out_ratio"]


def test_abi_entry_follows_the_conventions():
    from test_abi import _ctype_of, _declared
    from grafp_amd import _lib
    d = _declared()
    ret, args = d["grafp_identify_tempo_f32"]
    assert ret == "int" and args[-1].startswith("grafp_stream_t")
    dense = d["grafp_identify_f32"][1]
    assert [a for a in args if a not in NEW_ARGS] == dense and all(a in args for a in NEW_ARGS)
    assert args.index("const int32_t *ratio_num") == dense.index("int min_overlap") + 1
    assert args[-2] == "int32_t *out_ratio"
    res, argtypes = _lib.SIGNATURES["grafp_identify_tempo_f32"]
    assert res is ctypes.c_int and [_ctype_of(a) for a in args] == list(argtypes)
    assert d["grafp_identify_tempo_workspace"] == ("size_t", ["int n_items", "int n_ratios", "int top"])
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "grafp_identify_tempo_f32") and hasattr(raw, "grafp_identify_tempo_workspace")


def test_workspace_is_sixteen_bytes_per_ratio_item_and_rank():
    from grafp_amd._lib import lib
    assert lib.grafp_identify_tempo_workspace(41, 15, 5) == 16 * 41 * 15 * 5
    assert lib.grafp_identify_tempo_workspace(4096, 64, 64) == 16 * 4096 * 64 * 64
    assert lib.grafp_identify_tempo_workspace(0, 3, 5) == 0
    assert lib.grafp_identify_tempo_workspace(4, 65, 5) == 0 and lib.grafp_identify_tempo_workspace(4, 0, 5) == 0
    assert lib.grafp_identify_tempo_workspace(4, 3, 65) == 0 and lib.grafp_identify_tempo_workspace(-1, 3, 5) == 0


def test_abi_entry_refuses_out_of_range_launches_without_a_gpu():
    from grafp_amd._lib import lib
    # never dereferenced: every call below fails an argument check before anything is launched (no call here may pass
    # them -- this file also runs on machines with a GPU).  The ratios are host memory and are read.
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(12)]

    def call(max_len, k, top=5, n=100, ratios=(250, 256), n_ratios=None, first=fake[0]):
        nums = (ctypes.c_int32 * max(1, len(ratios)))(*ratios)
        return lib.grafp_identify_tempo_f32(first, n, fake[1], 2, fake[2], 1000, fake[3], k, fake[4], fake[5], 4,
                                            max_len, top, 0, ctypes.cast(nums, ctypes.c_void_p),
                                            len(ratios) if n_ratios is None else n_ratios, fake[10], fake[6], fake[7],
                                            fake[8], fake[9], fake[11], None)
    assert call(257, 4) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(8, 33) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(205, 40) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(8, 4, top=65) == -1 and b"top" in lib.grafp_last_error()
    assert call(257, 4, n_ratios=0) == -1 and b"n_ratios" in lib.grafp_last_error()
    assert call(257, 4, n_ratios=65) == -1 and b"n_ratios" in lib.grafp_last_error()
    assert call(257, 4, ratios=(127, 256)) == -1 and b"[128, 512]" in lib.grafp_last_error()
    assert call(257, 4, ratios=(256, 513)) == -1 and b"[128, 512]" in lib.grafp_last_error()
    assert call(257, 4, ratios=(256, 256)) == -1 and b"ascending" in lib.grafp_last_error()
    assert call(257, 4, ratios=(260, 250)) == -1 and b"ascending" in lib.grafp_last_error()
    assert call(8, 4, first=None) == -1 and b"null pointer" in lib.grafp_last_error()
    nums = (ctypes.c_int32 * 1)(256)
    assert lib.grafp_identify_tempo_f32(fake[0], 100, fake[1], 2, fake[2], 1000, fake[3], 4, fake[4], fake[5], 4, 8, 5,
                                        0, None, 1, fake[10], fake[6], fake[7], fake[8], fake[9], fake[11], None) == -1
    assert b"null pointer" in lib.grafp_last_error()
    assert lib.grafp_identify_tempo_f32(fake[0], 100, fake[1], 2, fake[2], 1000, fake[3], 4, fake[4], fake[5], 4, 8, 5,
                                        0, ctypes.cast(nums, ctypes.c_void_p), 1, fake[10], fake[6], fake[7], fake[8],
                                        fake[9], None, None) == -1
    assert b"null pointer" in lib.grafp_last_error()


def test_identify_tempo_kernels_have_no_packed_f32_instructions():
    """The shipped object's own command (make -n), compiled to device assembly: both query-row plans of pass 1 and the
    merge of pass 2 are there, nothing else, and none holds a packed-f32 instruction."""
    asm = shipped_asm("identify_tempo")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert sum("identify_tempo_kernel" in k for k in kernels) == 2
    assert sum("identify_tempo_merge_kernel" in k for k in kernels) == 1 and len(kernels) == 3
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm


def test_query_takes_a_tempo_on_the_command_line(capsys):
    from grafp_amd import identify
    with pytest.raises(SystemExit) as e:
        identify.main(["query", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--tempo" in out and "--tempo-step" in out
