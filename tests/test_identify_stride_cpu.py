"""CPU tests of identification from every Q-th segment of the recording (csrc/identify_stride.hip, ops.identify_stride,
FingerprintLibrary.identify(query_stride=Q), StreamMonitor(query_stride=Q)).  The contract is identify_tempo.hip's at the
single ratio 256 * Q, where w(s) = s * Q exactly, so the numpy restatement is tests/_identify_tempo_ref.py's: here it is
checked on hand-built cases, next to kept_items, the refusal paths, the monitor's bookkeeping, the C ABI entry, the
shipped assembly and the command line.  No GPU call is made."""
import ctypes
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _identify_ref import identify_ref, score_run
from _identify_tempo_ref import tempo_case, tempo_item, tempo_ref, w
from grafp_amd import library, monitor, ops
from grafp_amd.util import load_config

NAMES = ("track", "offset", "score", "votes")


def _rows(n, seed):
    """Dyadic rows (multiples of 2^-8 in [-1/8, 1/8)): every product and partial sum is exact in f32."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-32, 32, size=(n, 128)) / 256.0).astype(np.float32)


def stride_item(rows, first, q, ids, Q, top=5, min_overlap=None):
    """One item through the restatement at the ratio 256 * Q -> [(track, offset, score, votes)]."""
    return [r[:4] for r in tempo_item(rows, first, q, ids, [256 * Q], top, min_overlap)]


# ---- the restatement ----------------------------------------------------------------------------------------------
def test_the_ratio_256_q_steps_q_rows_exactly():
    for Q in range(1, 33):
        assert np.array_equal(w(np.arange(256), 256 * Q), np.arange(256) * Q)


@pytest.mark.parametrize("min_overlap", [None, 1, 3])
def test_stride_one_is_the_dense_restatement(min_overlap):
    rows, first, q, ids, item_row, item_len = tempo_case(5 + (min_overlap or 0), [256], 64, 40, 6)
    got = tempo_ref(rows, first, q, ids, item_row, item_len, [256], top=8, min_overlap=min_overlap)[:4]
    want = identify_ref(rows, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap)
    for g, x, name in zip(got, want, NAMES):
        assert np.array_equal(g, x), name
    assert (got[0][:, 0] >= 0).sum() > 40


def test_negative_alignment_with_stride_three():
    rows, first = _rows(12, 2), [0, 12]
    q = np.concatenate([_rows(1, 3), rows[[0, 3, 6]]])            # kept row 0 sits three rows before the track
    ids = np.array([[-1], [0], [3], [6]])
    assert stride_item(rows, first, q, ids, 3) == []              # 3 pairs of the min(4, 12 // 3) it needs
    res = stride_item(rows, first, q, ids, 3, min_overlap=3)
    assert [(t, o, v) for t, o, _, v in res] == [(0, -3, 3)]
    assert res[0][2] == score_run(q[1:4], rows[[0, 3, 6]])


def test_run_across_a_track_boundary_is_rejected_or_clipped():
    rows, first = _rows(12, 4), [0, 6, 12]
    q = rows[[2, 4, 6, 8]].copy()                                 # alignment 2 at Q = 2: rows 2, 4 | 6, 8
    ids = np.array([[2], [4], [6], [8]])
    # default: need = 4, each track holds 2 pairs and could always hold 6 // 2 = 3 -> neither eligible
    assert stride_item(rows, first, q, ids, 2) == []
    res = stride_item(rows, first, q, ids, 2, min_overlap=2)
    assert {(t, o, v) for t, o, _, v in res} == {(0, 2, 2), (1, -4, 2)}
    by_track = {t: s for t, _, s, _ in res}
    assert by_track[0] == score_run(q[0:2], rows[[2, 4]]) and by_track[1] == score_run(q[2:4], rows[[6, 8]])


def test_track_with_fewer_rows_than_need():
    rows, first = _rows(16, 6), [0, 4, 16]
    q = rows[[0, 2, 4, 6, 8]].copy()
    ids = np.array([[0], [2], [4], [6], [8]])
    res = stride_item(rows, first, q, ids, 2)                     # need = 5
    # track 0 is eligible through cap = max(1, 4 // 2) = 2; track 1 holds 3 pairs of the min(5, 12 // 2) it needs
    assert [(t, o, v) for t, o, _, v in res] == [(0, 0, 2)]
    assert res[0][2] == score_run(q[0:2], rows[[0, 2]])
    res = stride_item(rows, first, q, ids, 2, min_overlap=3)
    assert sorted((t, o, v) for t, o, _, v in res) == [(0, 0, 2), (1, -4, 3)]
    # a track shorter than the stride can always hold one pair: cap = max(1, 1 // 4)
    res = stride_item(_rows(3, 7), [0, 1, 3], _rows(3, 7)[[0, 0, 0]], np.array([[0], [-1], [-1]]), 4)
    assert [(t, o, v) for t, o, _, v in res] == [(0, 0, 1)]


def test_equal_scores_smaller_offset_then_smaller_track():
    base, filler = _rows(2, 8), _rows(2, 9)
    track = np.stack([base[0], filler[0], base[1], filler[1]] * 2)       # base at rows 0, 2 and at rows 4, 6
    rows, first = np.concatenate([track, track]), [0, 8, 16]
    ids = np.array([[0, 4, 8, 12], [2, 6, 10, 14]])
    res = stride_item(rows, first, base, ids, 2, top=5)
    assert [(t, o) for t, o, _, _ in res] == [(0, 0), (1, 0)]
    assert res[0][2] == res[1][2] == score_run(base, base)


# ---- kept_items ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 2, 3, 4, 5])
def test_kept_items_is_the_brute_force_filter(Q):
    rows = np.array([j for j in range(0, 23) for _ in range(8)], np.int64)
    lens = np.array([n for _ in range(0, 23) for n in (0, 1, 2, Q - 1, Q, Q + 1, 7, 31)], np.int32)
    kept_row, kept_len = library.kept_items(rows, lens, Q)
    assert kept_row.dtype == np.int64 and kept_len.dtype == np.int32
    for j, n, c0, cnt in zip(rows, lens, kept_row, kept_len):
        seg = np.arange(j, j + n)
        want = seg[seg % Q == 0] // Q                               # the kept rows inside the item
        assert cnt == len(want), (j, n)
        assert c0 == -(-j // Q)
        if cnt:
            assert want.tolist() == list(range(c0, c0 + cnt)), (j, n)
    if Q > 1:                                                       # off the grid and shorter than the stride: nothing
        assert library.kept_items([1], [Q - 1], Q)[1].tolist() == [0]
    assert library.kept_items([Q], [1], Q)[1].tolist() == [1]


# ---- the library ----------------------------------------------------------------------------------------------------
def _tiny_model():
    from grafp_amd.train import build_model
    torch.manual_seed(0)
    return build_model(load_config())


def _cpu_lib(model):
    rows = torch.from_numpy(_rows(14, 13))
    return library.FingerprintLibrary(model, load_config(), rows, [0, 0, 7, 8, 14], ["a", "b", "c", "d"],
                                      precision="f32", device="cpu")


def _compact_lib(model):
    quantiser = {"centroids": torch.zeros(2, 128), "codebooks": torch.zeros(16, 256, 8)}
    return library.FingerprintLibrary.from_codes(model, load_config(), quantiser, torch.zeros(14, dtype=torch.int32),
                                                 torch.zeros((14, 16), dtype=torch.uint8), [0, 0, 7, 8, 14],
                                                 ["a", "b", "c", "d"], precision="f32", device="cpu")


def test_a_query_stride_is_refused_where_it_is_not_built():
    model = _tiny_model()
    lib, wave = _cpu_lib(model), np.zeros(16000, np.float32)
    for call in (lib.identify, lib.identify_windows):
        with pytest.raises(NotImplementedError, match="query_stride"):
            call(wave, query_stride=2, tempo=0.05)
        with pytest.raises(NotImplementedError, match="query_stride"):
            call.__func__(lib.thin(2), wave, query_stride=2)
        with pytest.raises(NotImplementedError, match="query_stride"):
            call.__func__(_compact_lib(model), wave, query_stride=2)
        for bad in (0, 33, -1, 2.5):
            with pytest.raises(ValueError, match="query_stride"):
                call(wave, query_stride=bad)
    with pytest.raises(NotImplementedError, match="query_stride"):
        monitor.StreamMonitor(lib.thin(2), 1, query_stride=2)
    with pytest.raises(ValueError, match="query_stride"):
        monitor.StreamMonitor(lib, 1, query_stride=33)
    for name in ("match", "self_matches"):                           # these do not take the option
        with pytest.raises(TypeError, match="query_stride"):
            getattr(lib, name)(wave, query_stride=2)


def test_query_stride_one_is_routed_as_without_it(monkeypatch):
    """At query_stride = 1 the front cuts the same segments, builds the same items and calls the hook with q_stride 1,
    on which FingerprintLibrary launches ops.identify; above 1 the hook gets every Q-th segment, the kept items and
    min_overlap // Q, and launches ops.identify_stride."""
    lib = _cpu_lib(_tiny_model())
    n_mels, n_frames = lib.settings["n_mels"], lib.settings["n_frames"]
    dense = torch.arange(45, dtype=torch.float32)[:, None, None].expand(45, n_mels, n_frames)
    monkeypatch.setattr(lib, "segments", lambda wav: dense)
    monkeypatch.setattr(lib, "_load_queries", lambda queries, fs: [torch.zeros(45 * 1536 + 14000)])
    monkeypatch.setattr(lib, "_embed", lambda segs: segs[:, :1, 0].repeat(1, 128).contiguous())
    monkeypatch.setattr(lib, "_search_rows", lambda q, k: torch.zeros((q.shape[0], 3), dtype=torch.int64))
    calls = []

    def hook(q, ids, item_row, item_len, top, min_overlap, max_len, nums=None, q_stride=1):
        calls.append((q[:, 0].tolist(), item_row.tolist(), item_len.tolist(), min_overlap, max_len, nums, q_stride))
        pad = lambda v, dt: torch.full((len(item_row), top), v, dtype=dt)
        return pad(-1, torch.int32), pad(0, torch.int32), pad(0.0, torch.float32), pad(0, torch.int32)
    monkeypatch.setattr(lib, "_identify_lists", hook)
    wave = np.zeros(16000, np.float32)
    assert lib.identify(wave, min_overlap=7) == lib.identify(wave, min_overlap=7, query_stride=1) == []
    assert calls[0] == calls[1] == (list(range(45)), [0], [45], 7, 45, None, 1)
    lib.identify(wave, min_overlap=7, query_stride=4)
    assert calls[2] == (list(range(0, 45, 4)), [0], [12], 1, 12, None, 4)
    lib.identify(wave, query_stride=2)
    assert calls[3][3] is None and calls[3][6] == 2
    del calls[:]
    plain = lib.identify_windows(wave)
    assert lib.identify_windows(wave, query_stride=1) == plain and calls[0] == calls[1] and calls[0][6] == 1
    _, jrow, jlen = library.window_items(45, 45 * 1536 + 14000, lib.settings)
    assert calls[0][1] == jrow.tolist() and calls[0][2] == jlen.tolist()
    strided = lib.identify_windows(wave, query_stride=4)
    krow, klen = library.kept_items(jrow, jlen, 4)
    assert calls[2][:3] == (list(range(0, 45, 4)), krow.tolist(), klen.tolist()) and calls[2][6] == 4
    assert [x["start_s"] for x in strided] == [x["start_s"] for x in plain]
    assert [x["segment_start_s"] for x in strided] == [int(k) * 4 * lib.segment_s for k in krow]
    # the hook's launch: the dense op at 1, the strided op above it (both refuse a CPU tensor by their own name)
    monkeypatch.undo()
    args = (torch.zeros(3, 128), torch.zeros((3, 2), dtype=torch.int64), np.zeros(1, np.int64), np.full(1, 3, np.int32),
            5, None, 3)
    for q_stride, op in ((1, "identify"), (2, "identify_stride")):
        seen = []
        monkeypatch.setattr(ops, op, lambda *a, **kw: seen.append((a, kw)) or "launched")
        assert lib._identify_lists(*args, None, q_stride) == "launched" and len(seen) == 1
        assert (seen[0][0][6:] == (2,)) if q_stride == 2 else (len(seen[0][0]) == 6)
        monkeypatch.undo()


def test_a_window_without_a_kept_row_keeps_its_start_and_has_no_matches(monkeypatch):
    lib = _cpu_lib(_tiny_model())
    monkeypatch.setattr(lib, "segments", lambda wav: torch.zeros(2, lib.settings["n_mels"], lib.settings["n_frames"]))
    monkeypatch.setattr(lib, "_load_queries", lambda queries, fs: [torch.zeros(60000)])
    monkeypatch.setattr(library, "window_items",
                        lambda *a, **kw: (np.array([0.0, 1.0]), np.array([0, 1], np.int64), np.array([0, 1], np.int32)))
    res = lib.identify_windows(np.zeros(1), query_stride=2)          # window 1 is segment 1 alone: off the grid
    assert [x["matches"] for x in res] == [[], []]
    assert [x["segment_start_s"] for x in res] == [0.0, lib.segment_s]


# ---- the monitor's bookkeeping --------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 2, 3, 4])
def test_monitor_files_the_kept_rows_and_identifies_the_kept_items(Q, monkeypatch):
    """push_rows in uneven pieces: every due window's item is kept_items of it over rows that are exactly the stream's
    segments c0 * Q, (c0 + 1) * Q, ...; what it reports is the schedule of window_items; the rows off the grid (NaN) never
    reach the search."""
    cfg = load_config()
    lib = library.FingerprintLibrary(None, cfg, torch.from_numpy(_rows(6, 1)), [0, 6], ["a"], precision="f32",
                                     device="cpu")
    n_seg = 131
    n_samples = monitor.samples_lower_bound(n_seg, cfg) + 700
    assert library.n_segments(n_samples, cfg) == n_seg
    dense = np.full((n_seg, 128), np.nan, np.float32)
    dense[::Q] = np.arange(0, n_seg, Q, dtype=np.float32)[:, None]
    searched, items = [], []

    def search(q, k):
        assert not torch.isnan(q).any()
        searched.extend(q[:, 0].tolist())
        return torch.zeros((q.shape[0], 2), dtype=torch.int64)

    def identify(q, ids, item_row, item_len, top, min_overlap, max_len=None, q_stride=1):
        assert q_stride == Q and max_len == -(-mon.per_window // Q) and q.shape[0] == ids.shape[0]
        for r, n in zip(item_row, item_len):
            items.append(q[int(r):int(r) + int(n), 0].tolist())
        return [[{"track": 0, "name": "a", "offset": 0, "offset_s": 0.0, "score": 1.0, "votes": 1}] if n else []
                for n in item_len]
    monkeypatch.setattr(lib, "_search_rows", search)
    monkeypatch.setattr(lib, "_identify_items", identify)
    mon = monitor.StreamMonitor(lib, 2, window_s=3.0, hop_s=1.0, query_stride=Q)
    rng, pos, got = np.random.RandomState(Q), 0, []
    while pos < n_seg:
        n = min(n_seg - pos, int(rng.randint(1, 12)))
        got += mon.push_rows([None, torch.from_numpy(dense[pos:pos + n])])[1]
        pos += n
        held = mon._first[2] - mon._first[1]
        assert held <= -(-(mon.per_window + 12 + 11) // Q) + 1            # the stale rows go: a window or so is kept
    got += mon.end(1, n_samples)
    starts, jrow, jlen = library.window_items(n_seg, n_samples, cfg, 3.0, 1.0)
    krow, klen = library.kept_items(jrow, jlen, Q)
    assert [x["start_s"] for x in got] == starts.tolist() and len(items) == len(got)
    for x, it, j, c0, cnt in zip(got, items, jrow, krow, klen):
        assert it == [float(v * Q) for v in range(c0, c0 + cnt)], (x["start_s"], it)
        assert x["segment_start_s"] == (int(c0) * Q if cnt else int(j)) * lib.segment_s
        assert bool(x["matches"]) == bool(cnt) and x["channel"] == 1
    assert searched == list(range(0, n_seg, Q))                           # every kept row once, no other
    assert mon.windows(1) == got


# ---- the op, the C ABI entry and the shipped object -------------------------------------------------------------
def test_identify_stride_op_refusals_without_a_gpu():
    rows = torch.zeros(8, 128)
    q = torch.zeros(300, 128)
    first = torch.tensor([0, 8])
    ids = torch.zeros(300, 4, dtype=torch.int64)
    one = torch.zeros(1, dtype=torch.int64)
    two = torch.tensor([2], dtype=torch.int32)
    assert ops.IDENTIFY_MAX_QUERY_STRIDE == 32
    with pytest.raises(ValueError, match="256 segments"):
        ops.identify_stride(rows, first, q, ids, one, torch.tensor([257], dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="k=33"):
        ops.identify_stride(rows, first, q, torch.zeros(300, 33, dtype=torch.int64), one, two, 2)
    with pytest.raises(ValueError, match="hits per item"):
        ops.identify_stride(rows, first, q, torch.zeros(300, 32, dtype=torch.int64), one, two, 2, max_len=257)
    with pytest.raises(ValueError, match="never decrease"):
        ops.identify_stride(rows, torch.tensor([0, 5, 3, 8]), q, ids, one, two, 2)
    with pytest.raises(ValueError, match="outside q_rows"):
        ops.identify_stride(rows, first, q, ids, torch.tensor([299]), two, 2)
    with pytest.raises(ValueError, match="top"):
        ops.identify_stride(rows, first, q, ids, one, two, 2, top=65)
    with pytest.raises(ValueError, match="min_overlap"):
        ops.identify_stride(rows, first, q, ids, one, two, 2, min_overlap=0)
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match=r"query_stride=.* not in \[1, 32\]"):
            ops.identify_stride(rows, first, q, ids, one, two, bad)
    # n + 255 * Q must stay below 2^32 (only the row count is read before the refusal: no such array exists)
    huge = torch.empty(((1 << 32) - 8000, 128), device="meta")
    with pytest.raises(ValueError, match="2\\^32"):
        ops.identify_stride(huge, torch.tensor([0, (1 << 32) - 8000]), q, ids, one, two, 32)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.identify_stride(rows, first, q, ids, one, two, 2)


def test_abi_entry_follows_the_conventions():
    from test_abi import _ctype_of, _declared
    from grafp_amd import _lib
    d = _declared()
    ret, args = d["grafp_identify_stride_f32"]
    assert ret == "int" and args[-1].startswith("grafp_stream_t")
    dense = d["grafp_identify_f32"][1]
    assert [a for a in args if a != "int query_stride"] == dense and args.index("int query_stride") == 4
    assert [a.replace("query_stride", "row_stride") for a in args] == d["grafp_identify_thin_f32"][1]
    res, argtypes = _lib.SIGNATURES["grafp_identify_stride_f32"]
    assert res is ctypes.c_int and [_ctype_of(a) for a in args] == list(argtypes)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "grafp_identify_stride_f32")


def test_abi_entry_refuses_out_of_range_launches_without_a_gpu():
    from grafp_amd._lib import lib
    # never dereferenced: every call below fails an argument check before anything is launched (no call here may pass
    # them -- this file also runs on machines with a GPU)
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(10)]

    def call(max_len, k, top=5, n=100, stride=2):
        return lib.grafp_identify_stride_f32(fake[0], n, fake[1], 2, stride, fake[2], 1000, fake[3], k, fake[4],
                                             fake[5], 4, max_len, top, 0, fake[6], fake[7], fake[8], fake[9], None)
    assert call(257, 4) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(8, 33) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(205, 40) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(8, 4, top=65) == -1 and b"top" in lib.grafp_last_error()
    assert call(8, 4, stride=0) == -1 and b"query_stride" in lib.grafp_last_error()
    assert call(8, 4, stride=33) == -1 and b"query_stride" in lib.grafp_last_error()
    assert call(8, 4, n=0) == -1 and b"bad sizes" in lib.grafp_last_error()
    assert lib.grafp_identify_stride_f32(None, 100, fake[1], 2, 2, fake[2], 1000, fake[3], 4, fake[4], fake[5], 4, 8,
                                         5, 0, fake[6], fake[7], fake[8], fake[9], None) == -1
    assert b"null pointer" in lib.grafp_last_error()
    assert lib.grafp_identify_stride_f32(fake[0], 100, fake[1], 2, 2, fake[2], 1000, fake[3], 4, fake[4], fake[5], 4,
                                         8, 5, 0, fake[6], fake[7], fake[8], None, None) == -1
    assert b"null pointer" in lib.grafp_last_error()


def test_identify_stride_kernels_have_no_packed_f32_instructions():
    """The shipped object's own command (make -n), compiled to device assembly: both query-row plans are there and
    neither holds a packed-f32 instruction."""
    asm = shipped_asm("identify_stride")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert sum("identify_stride_kernel" in k for k in kernels) == 2 and len(kernels) == 2
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm


@pytest.mark.parametrize("cmd", ["query", "monitor"])
def test_the_command_line_takes_a_query_stride(cmd, capsys, monkeypatch):
    from grafp_amd import identify
    with pytest.raises(SystemExit) as e:
        identify.main([cmd, "--help"])
    assert e.value.code == 0
    assert "--query-stride" in capsys.readouterr().out
    seen = {}

    class Stop(Exception):
        pass

    def parse(self, argv=None):
        seen["args"] = real(self, argv)
        raise Stop
    import argparse
    real = argparse.ArgumentParser.parse_args
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    tail = ["--library", "LIB", "a.wav"] if cmd == "query" else ["LIB", "a.wav"]
    with pytest.raises(Stop):
        identify.main([cmd, "--ckp", "m.pth", "--query-stride", "4"] + tail)
    assert seen["args"].query_stride == 4
    with pytest.raises(Stop):
        identify.main([cmd, "--ckp", "m.pth"] + tail)
    assert seen["args"].query_stride == 1
