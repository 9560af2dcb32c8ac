"""CPU tests of the sharded fingerprint library (grafp_amd/sharded.py, csrc/merge_lists.hip, ops.merge_track_lists): the
numpy restatement of the merge on hand-built lists, the split rule, the tables, the files, the refusals, the C ABI
entry, the shipped assembly and the command line.  No GPU call is made."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _shard_ref import merge_ref, random_lists
from grafp_amd import library, ops
from grafp_amd.sharded import ShardedFingerprintLibrary, split_tracks
from test_identify_tempo_cpu import _cpu_lib

INT_MIN = -2 ** 31
NINF = -np.inf


# ---- the restatement ----------------------------------------------------------------------------------------------
def _lists(S, top, P, pad):
    track = np.full((S, 1, top), -1, np.int32)
    score = np.full((S, 1, top), NINF, np.float32)
    payload = np.empty((P, S, 1, top), np.int32)
    for p in range(P):
        payload[p] = pad[p]
    return track, score, payload


def test_equal_scores_in_two_shards_go_to_the_smaller_global_track():
    pad = [INT_MIN, 0]
    track, score, payload = _lists(2, 3, 2, pad)
    track[0, 0, :2], score[0, 0, :2] = [4, 1], [0.9, 0.5]                   # global 4, 1
    track[1, 0, :2], score[1, 0, :2] = [0, 2], [0.9, 0.5]                   # global 5, 7
    payload[0, 0, 0, :2], payload[0, 1, 0, :2] = [10, 11], [20, 21]
    payload[1, 0, 0, :2], payload[1, 1, 0, :2] = [3, 4], [5, 6]
    t, s, p = merge_ref(track, score, payload, [0, 5], pad)
    assert t.tolist() == [[4, 5, 1]] and s.tolist() == [[np.float32(0.9), np.float32(0.9), 0.5]]
    assert p[0].tolist() == [[10, 20, 11]] and p[1].tolist() == [[3, 5, 4]]
    # the same entries with the shards' contents exchanged: the global track decides, not the shard
    t2, _, _ = merge_ref(track[::-1], score[::-1], payload[:, ::-1], [0, 5], pad)
    assert t2.tolist() == [[0, 9, 2]]


def test_padding_is_skipped_and_short_lists_leave_each_payloads_own_pad():
    pad = [INT_MIN, 0, -1, 7]
    track, score, payload = _lists(3, 4, 4, pad)
    track[0, 0, 0], score[0, 0, 0], payload[:, 0, 0, 0] = 2, 0.25, [1, 2, 3, 4]
    track[2, 0, 0], score[2, 0, 0], payload[:, 2, 0, 0] = 0, 0.75, [5, 6, 7, 8]
    score[1, 0, :] = 5.0                                                     # a padding entry's score is never read
    t, s, p = merge_ref(track, score, payload, [0, 3, 3], pad)
    assert t.tolist() == [[3, 2, -1, -1]] and s.tolist() == [[0.75, 0.25, NINF, NINF]]
    assert p[:, 0, :].tolist() == [[5, 1, INT_MIN, INT_MIN], [6, 2, 0, 0], [7, 3, -1, -1], [8, 4, 7, 7]]


def test_the_overflow_mark_goes_to_slot_zero():
    pad = [INT_MIN, -1, 0, 0]
    track, score, payload = _lists(2, 3, 4, pad)
    track[0, 0, :2], score[0, 0, :2] = [1, 0], [0.5, 0.25]
    track[1, 0, 0] = -2
    t, s, p = merge_ref(track, score, payload, [0, 4], pad)
    assert t.tolist() == [[-2, -1, -1]] and (s == NINF).all()
    assert all((p[j] == pad[j]).all() for j in range(4))


def test_one_shard_is_the_identity_and_random_lists_are_in_the_ops_order():
    track, score, payload, base, pad = random_lists(3, 1, 12, 6, 3, keep=0.7)
    t, s, p = merge_ref(track, score, payload, base, pad)
    assert np.array_equal(t, track[0]) and np.array_equal(s, score[0]) and np.array_equal(p, payload[:, 0])
    track, score, payload, base, pad = random_lists(4, 5, 20, 6, 2)
    t, s, _ = merge_ref(track, score, payload, base, pad)
    assert (t >= 0).all() and (np.diff(s, axis=1) <= 0).all()
    ties = np.diff(s, axis=1) == 0
    assert ties.any() and (np.diff(t, axis=1)[ties] > 0).all()               # equal scores: global track ascending


# ---- the split rule and the tables ------------------------------------------------------------------------------
def test_split_rule_on_a_small_table():
    first = [0, 0, 7, 8, 14]
    assert split_tracks(first, 1).tolist() == [0, 4]
    assert split_tracks(first, 2).tolist() == [0, 2, 4]                      # 7 rows each
    assert split_tracks(first, 3).tolist() == [0, 2, 4, 4]                   # cuts at rows 4.67 -> 7 and 9.33 -> 14
    assert split_tracks(first, 4).tolist() == [0, 2, 2, 4, 4]                # 3.5 -> 7, 7 -> 7, 10.5 -> 14
    assert split_tracks(first, 6).tolist() == [0, 2, 2, 2, 4, 4, 4]
    assert split_tracks([0], 3).tolist() == [0, 0, 0, 0]                     # no tracks at all
    with pytest.raises(ValueError, match="n_shards"):
        split_tracks(first, 0)


@pytest.mark.parametrize("S", [1, 2, 3, 4, 6])
def test_split_keeps_tracks_whole_and_the_tables_consistent(S):
    lib = _cpu_lib()
    sh = ShardedFingerprintLibrary.split(lib, S)
    assert len(sh.shards) == S and sh.tb.tolist() == split_tracks(lib.first, S).tolist()
    assert sh.rb.tolist() == [int(lib.first[t]) for t in sh.tb]             # boundaries only at tracks
    assert np.array_equal(sh.first, lib.first) and sh.names == lib.names == ["a", "b", "c", "d"]
    assert (sh.n_tracks, sh.n_rows, sh.row_stride, sh.step, sh.segment_s) == (4, 14, 1, lib.step, lib.segment_s)
    assert sh.settings == lib.settings and sh.device == lib.device and sh.precision == "f32"
    for s, part in enumerate(sh.shards):
        t0, t1 = int(sh.tb[s]), int(sh.tb[s + 1])
        assert part.names == lib.names[t0:t1] and part.n_tracks == t1 - t0
        assert np.array_equal(part.first, lib.first[t0:t1 + 1] - lib.first[t0])
        assert torch.equal(part.rows(), lib.rows()[int(sh.rb[s]):int(sh.rb[s + 1])])
    assert any(part.n_rows == 0 for part in sh.shards) == (S >= 3)           # empty shards from S = 3 on
    assert [s for s, _ in sh._live()] == [s for s in range(S) if sh.rb[s + 1] > sh.rb[s]]
    assert sh.nbytes == sum(part.nbytes for part in sh.shards)


def test_split_of_a_thinned_library_keeps_the_row_stride():
    thin = _cpu_lib().thin(2)
    sh = ShardedFingerprintLibrary.split(thin, 2)
    assert sh.row_stride == 2 and all(part.row_stride == 2 for part in sh.shards)
    assert np.array_equal(sh.first, thin.first) and sh.tb.tolist() == split_tracks(thin.first, 2).tolist()
    assert torch.equal(torch.cat([part.rows() for part in sh.shards]), thin.rows())


def test_refusals_of_the_sharded_library():
    lib = _cpu_lib()
    quantiser = {"centroids": torch.zeros(2, 128), "codebooks": torch.zeros(16, 256, 8)}
    compact = library.FingerprintLibrary.from_codes(lib.model, lib.settings, quantiser, torch.zeros(3, dtype=torch.int32),
                                                    torch.zeros(3, 16, dtype=torch.uint8), [0, 3], ["x"],
                                                    precision="f32", device="cpu")
    with pytest.raises(NotImplementedError, match="compact"):
        ShardedFingerprintLibrary.split(compact, 2)
    with pytest.raises(NotImplementedError, match="compact"):
        ShardedFingerprintLibrary([compact])
    sh = ShardedFingerprintLibrary.split(lib.thin(2), 2)
    with pytest.raises(NotImplementedError, match="tempo"):
        sh.identify(np.zeros(16000, np.float32), tempo=0.06)
    with pytest.raises(NotImplementedError, match="tempo"):
        sh.identify_windows(np.zeros(64000, np.float32), tempo=0.06)
    with pytest.raises(NotImplementedError, match="every row"):
        sh.match(np.zeros(64000, np.float32))
    with pytest.raises(NotImplementedError, match="self_matches"):
        ShardedFingerprintLibrary.split(lib, 2).self_matches()
    with pytest.raises(ValueError, match="devices"):
        ShardedFingerprintLibrary.split(lib, 3, devices=["cpu", "cpu"])
    with pytest.raises(ValueError, match="65 shards"):
        ShardedFingerprintLibrary.split(lib, 65)


def test_timeline_is_the_librarys():
    from test_identify_tempo_cpu import _windows
    lib = _cpu_lib()
    sh = ShardedFingerprintLibrary.split(lib, 3)
    windows = _windows(266 / 256, 12, lib.segment_s, tempo=True)
    assert sh.timeline(windows) == lib.timeline(windows)


def test_both_libraries_answer_with_the_same_front():
    assert issubclass(ShardedFingerprintLibrary, library.LibraryFront)
    assert issubclass(library.FingerprintLibrary, library.LibraryFront)
    assert not issubclass(ShardedFingerprintLibrary, library.FingerprintLibrary)
    for name in ("identify", "identify_windows", "timeline", "match", "_identify_items", "_match_rows", "_match_entry",
                 "_load_queries", "_embed", "segments", "_search_and_identify", "_check_item_len", "_fingerprint_tracks",
                 "_need_dense", "_need_flat", "_need_tempo_form"):
        assert getattr(ShardedFingerprintLibrary, name) is getattr(library.FingerprintLibrary, name), name
        assert getattr(ShardedFingerprintLibrary, name) is getattr(library.LibraryFront, name), name
    for name in ("_search_rows", "_identify_lists", "_match_lists"):           # the hooks: each library's own
        own = {vars(cls)[name] for cls in (library.LibraryFront, library.FingerprintLibrary, ShardedFingerprintLibrary)}
        assert len(own) == 3, name
    assert ShardedFingerprintLibrary.is_compact is False


def test_a_front_without_hooks_refuses_at_the_search():
    lib = _cpu_lib()
    reached = []

    class Bare(library.LibraryFront):
        def segments(self, wav):
            return torch.zeros((3, 4, 4))

        def _embed(self, segs):
            reached.append(int(segs.shape[0]))
            return torch.zeros((segs.shape[0], 128))

    bare = Bare(lib.model, lib.settings, "f32", torch.device("cpu"), 1)
    assert (bare.n_tracks, bare.n_rows, bare.names, bare.row_stride, bare.settings) == (0, 0, [], 1, lib.settings)
    assert bare.identify(np.zeros(16000, np.float32)) == [] and reached == []   # no rows: nothing to search
    bare.first, bare.names = lib.first, lib.names
    with pytest.raises(NotImplementedError):
        bare.identify(np.zeros(16000, np.float32))
    assert reached == [3]                                                    # embedded, then refused at _search_rows
    q, ids = torch.zeros((3, 128)), torch.zeros((3, 2), dtype=torch.int64)
    for call in (lambda: bare._search_rows(q, 2), lambda: bare.is_compact,
                 lambda: bare._identify_lists(q, ids, np.zeros(1, np.int64), np.full(1, 3, np.int32), 5, None, 3),
                 lambda: bare._match_lists(q, torch.tensor([0, 3]), 2, None, {})):
        with pytest.raises(NotImplementedError):
            call()


# ---- files --------------------------------------------------------------------------------------------------------
def test_save_and_load_round_trip(tmp_path):
    lib = _cpu_lib()
    sh = ShardedFingerprintLibrary.split(lib, 3)                             # the third shard is empty
    out = str(tmp_path / "lib")
    sh.save(out)
    meta = json.load(open(os.path.join(out, "shards.json")))
    assert meta["format"] == 1 and meta["n_shards"] == 3 and meta["tb"] == [0, 2, 4, 4]
    assert meta["shards"] == ["shard000", "shard001", "shard002"]
    assert meta["model_digest"] == library.model_digest(lib.model)
    assert all(os.path.exists(os.path.join(out, d, "library.json")) for d in meta["shards"])
    assert ShardedFingerprintLibrary.is_sharded_dir(out) and not ShardedFingerprintLibrary.is_sharded_dir(str(tmp_path))
    back = ShardedFingerprintLibrary.load(out, lib.model)
    assert back.tb.tolist() == sh.tb.tolist() and back.rb.tolist() == sh.rb.tolist()
    assert np.array_equal(back.first, lib.first) and back.names == lib.names
    assert back.settings == lib.settings and back.precision == "f32" and back.row_stride == 1
    for a, b in zip(back.shards, sh.shards):
        assert torch.equal(a.rows(), b.rows()) and np.array_equal(a.first, b.first) and a.names == b.names
    # a thinned one keeps its stride through the files
    thin = ShardedFingerprintLibrary.split(lib.thin(2), 2)
    thin.save(str(tmp_path / "thin"))
    assert ShardedFingerprintLibrary.load(str(tmp_path / "thin"), lib.model).row_stride == 2


def test_load_refuses_another_model_and_a_bad_table(tmp_path):
    from grafp_amd.train import build_model
    from grafp_amd.util import load_config
    lib = _cpu_lib()
    out = str(tmp_path / "lib")
    ShardedFingerprintLibrary.split(lib, 2).save(out)
    torch.manual_seed(1)
    other = build_model(load_config())
    with pytest.raises(ValueError, match="another model"):
        ShardedFingerprintLibrary.load(out, other)
    assert ShardedFingerprintLibrary.load(out, other, force=True).n_rows == 14
    path = os.path.join(out, "shards.json")
    good = json.load(open(path))
    for bad in ({"format": 2}, {"tb": [0, 4]}, {"tb": [0, 3, 2]}, {"tb": [1, 2, 4]}, {"shards": ["shard000"]},
                {"shards": ["shard000", "../elsewhere"]}, {"n_shards": 3}, {"shards": [], "tb": [0], "n_shards": 0}):
        json.dump({**good, **bad}, open(path, "w"))
        with pytest.raises(ValueError, match="shards.json"):
            ShardedFingerprintLibrary.load(out, lib.model)
    json.dump({**good, "tb": [0, 1, 4]}, open(path, "w"))                   # well formed, but not what the shards hold
    with pytest.raises(ValueError, match="shards.json says"):
        ShardedFingerprintLibrary.load(out, lib.model)


# ---- the op -------------------------------------------------------------------------------------------------------
def test_merge_track_lists_op_refusals_without_a_gpu():
    assert (ops.MERGE_LISTS_MAX, ops.MERGE_LISTS_MAX_SLOTS, ops.MERGE_LISTS_MAX_PAYLOAD) == (64, 4096, 6)

    def call(S=2, n_items=3, L=5, P=2, base=None, pad=None, **kw):
        track = torch.zeros((S, n_items, L), dtype=torch.int32)
        score = torch.zeros((S, n_items, L))
        payload = torch.zeros((P, S, n_items, L), dtype=torch.int32)
        return ops.merge_track_lists(track, score, payload, list(range(S)) if base is None else base,
                                     [0] * P if pad is None else pad, **kw)
    with pytest.raises(ValueError, match="S=65"):
        call(S=65, L=1)
    with pytest.raises(ValueError, match="S=0"):
        call(S=0)
    with pytest.raises(ValueError, match="top=65"):
        call(S=1, L=65)
    with pytest.raises(ValueError, match="top=0"):
        call(L=0)
    # (S <= 64 and top <= 64 imply the 4096 slots: the product's own refusal is never reached)
    with pytest.raises(ValueError, match="P=7"):
        call(P=7)
    with pytest.raises(ValueError, match="ascending"):
        call(base=[3, 2])
    with pytest.raises(ValueError, match="ascending"):
        call(base=[-1, 2])
    with pytest.raises(ValueError, match="track bases"):
        call(base=[0, 1, 2])
    with pytest.raises(ValueError, match="pads"):
        call(pad=[0])
    for top in (0, 6):                                                       # at most the length of the lists
        with pytest.raises(ValueError, match=f"top={top}"):
            call(top=top)
    with pytest.raises(ValueError, match="track and score"):
        ops.merge_track_lists(torch.zeros((2, 3, 5), dtype=torch.int32), torch.zeros((2, 3, 4)), None, [0, 1], [])
    with pytest.raises(ValueError, match="payload must be"):
        ops.merge_track_lists(torch.zeros((2, 3, 5), dtype=torch.int32), torch.zeros((2, 3, 5)),
                              torch.zeros((2, 2, 3, 4), dtype=torch.int32), [0, 1], [0, 0])
    with pytest.raises(RuntimeError, match="no CPU"):                        # after the host checks
        call(base=[0, 0])                                                    # (equal bases: an empty shard)
    with pytest.raises(RuntimeError, match="no CPU"):
        call(P=0)


# ---- the C ABI entry and the shipped object ---------------------------------------------------------------------
def test_abi_entry_follows_the_conventions():
    from test_abi import _ctype_of, _declared
    from grafp_amd import _lib
    ret, args = _declared()["grafp_merge_track_lists_f32"]
    assert ret == "int" and args[-1].startswith("grafp_stream_t") and len(args) == 13
    assert args[7:9] == ["const int32_t *track_base", "const int32_t *pad"]
    res, argtypes = _lib.SIGNATURES["grafp_merge_track_lists_f32"]
    assert res is ctypes.c_int and [_ctype_of(a) for a in args] == list(argtypes)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "grafp_merge_track_lists_f32") and raw.grafp_abi_version() == 1


def test_abi_entry_refuses_out_of_range_launches_without_a_gpu():
    from grafp_amd._lib import lib
    # never dereferenced: every call below fails an argument check before anything is launched, or has no item (no call
    # here may launch -- this file also runs on machines with a GPU).  track_base and pad are host memory and are read.
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(6)]

    def call(S=2, n_items=3, top=5, P=2, base=None, pad=(0, 0, 0, 0, 0, 0), ptrs=fake, null_base=False):
        base = list(range(max(S, 1))) if base is None else base
        c_base = (ctypes.c_int32 * len(base))(*base)
        c_pad = (ctypes.c_int32 * len(pad))(*pad)
        return lib.grafp_merge_track_lists_f32(ptrs[0], ptrs[1], ptrs[2], S, n_items, top, P,
                                               None if null_base else ctypes.cast(c_base, ctypes.c_void_p),
                                               ctypes.cast(c_pad, ctypes.c_void_p), ptrs[3], ptrs[4], ptrs[5], None)
    assert call(S=0) == -1 and b"n_lists" in lib.grafp_last_error()
    assert call(S=65) == -1 and b"n_lists" in lib.grafp_last_error()
    assert call(top=0) == -1 and b"top" in lib.grafp_last_error()
    assert call(top=65) == -1 and b"top" in lib.grafp_last_error()
    assert call(S=64, top=64, n_items=0) == 0                                # the 4096 slots themselves are taken
    assert call(P=-1) == -1 and b"n_payload" in lib.grafp_last_error()
    assert call(P=7) == -1 and b"n_payload" in lib.grafp_last_error()
    assert call(n_items=-1) == -1 and b"n_items" in lib.grafp_last_error()
    assert call(base=[3, 2]) == -1 and b"ascending" in lib.grafp_last_error()
    assert call(base=[-1, 2]) == -1 and b"ascending" in lib.grafp_last_error()
    for missing in (0, 1, 2, 3, 4, 5):
        ptrs = [None if i == missing else p for i, p in enumerate(fake)]
        assert call(ptrs=ptrs) == -1 and b"null pointer" in lib.grafp_last_error(), missing
    assert call(null_base=True) == -1 and b"null pointer" in lib.grafp_last_error()
    assert call(n_items=0) == 0 and call(n_items=0, base=[4, 4]) == 0       # nothing to launch: success
    ptrs = [fake[0], fake[1], None, fake[3], fake[4], None]
    assert call(n_items=0, P=0, ptrs=ptrs) == 0                              # without payloads their pointers may be null


def test_merge_kernel_has_no_packed_f32_instructions():
    """The shipped object's own command (make -n), compiled to device assembly: the one merge kernel, nothing else, and
    no packed-f32 instruction."""
    asm = shipped_asm("merge_lists")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert len(kernels) == 1 and "merge_track_lists_kernel" in kernels[0]
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "ds_" in asm                                                      # the sort runs in LDS


def test_build_takes_shards_on_the_command_line(capsys):
    from grafp_amd import identify
    with pytest.raises(SystemExit) as e:
        identify.main(["build", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--shards" in out and "--devices" in out
