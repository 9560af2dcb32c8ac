"""CPU tests of identification against a library that keeps every D-th fingerprint row (csrc/identify_thin.hip,
ops.identify_thin, FingerprintLibrary.row_stride): the numpy restatement on hand-built cases, thin(), the files, the
refusal paths, the C ABI entry, the shipped assembly and the command line.  No GPU call is made."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _identify_ref import identify_ref, score_run
from _identify_thin_ref import pairs_of, thin_case, thin_first, thin_item, thin_ref, thin_rows
from grafp_amd import library, ops
from grafp_amd.util import load_config


def _rows(n, seed):
    """Dyadic rows (multiples of 2^-8 in [-1/8, 1/8)): every product and partial sum is exact in f32."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-32, 32, size=(n, 128)) / 256.0).astype(np.float32)


# ---- the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_overlap", [None, 1, 3])
def test_stride_one_is_the_dense_restatement(min_overlap):
    rows, first, q, ids, item_row, item_len = thin_case(5 + (min_overlap or 0), 1, n_items=40, max_ql=24)
    got = thin_ref(rows, first, q, ids, item_row, item_len, 1, top=8, min_overlap=min_overlap)
    want = identify_ref(rows, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap)
    for g, w, name in zip(got, want, ("track", "offset", "score", "votes")):
        assert np.array_equal(g, w), name
    assert (got[0][:, 0] >= 0).sum() > 20


def test_thinning_keeps_every_dth_row_of_every_track():
    first = np.array([0, 0, 7, 8, 14])
    rows = _rows(14, 1)
    kept, kfirst = thin_rows(rows, first, 3)
    assert kfirst.tolist() == [0, 0, 3, 4, 6] == thin_first(first, 3).tolist()
    assert np.array_equal(kept, rows[[0, 3, 6, 7, 8, 11]])
    assert pairs_of(-2, 0, 4, 7, 3) == [2, 5] and pairs_of(4, 0, 4, 7, 3) == [2, 5] and pairs_of(0, 1, 2, 9, 3) == [3]


def test_negative_alignment_with_stride_three():
    dense = _rows(12, 2)
    rows, first = thin_rows(dense, [0, 12], 3)                    # kept: dense 0, 3, 6, 9
    q = np.concatenate([_rows(2, 3), dense[0:5]])                 # query row 0 sits at fine position -2
    ids = np.array([[-1], [-1], [0], [0], [-1], [1], [-1]])       # s = 3 -> row 0: the neighbouring alignment -3
    res = thin_item(rows, first, q, ids, 3)
    assert [(t, o, v) for t, o, _, v in res] == [(0, -2, 2)]      # pairs s = 2, 5 on rows 0, 1; need = 7 // 3 = 2
    assert res[0][2] == score_run(q[[2, 5]], rows[0:2])
    # a = -3 pairs s = 3, 6 with rows 0, 1: it has one vote and loses to the exact alignment on score
    both = thin_item(rows, first, q, ids, 3, top=5)
    assert len(both) == 1


def test_run_across_a_track_boundary_is_rejected_or_clipped():
    dense = _rows(12, 4)
    rows, first = thin_rows(dense, [0, 6, 12], 2)                 # 3 kept rows per track
    assert first.tolist() == [0, 3, 6]
    q = _rows(8, 5)
    q[[0, 2, 4, 6]] = rows[1:5]                                   # fine alignment 2: rows 1, 2 | 3, 4
    ids = np.full((8, 1), -1)
    ids[[0, 2, 4, 6], 0] = [1, 2, 3, 4]
    # default: need = 8 // 2 = 4, each track holds only 2 pairs of its 3 rows -> neither eligible
    assert thin_item(rows, first, q, ids, 2) == []
    res = thin_item(rows, first, q, ids, 2, min_overlap=4)        # need = 2
    assert {(t, o, v) for t, o, _, v in res} == {(0, 2, 2), (1, -4, 2)}
    by_track = {t: s for t, _, s, _ in res}
    assert by_track[0] == score_run(q[[0, 2]], rows[1:3]) and by_track[1] == score_run(q[[4, 6]], rows[3:5])


def test_track_with_fewer_rows_than_need():
    dense = _rows(16, 6)
    rows, first = thin_rows(dense, [0, 4, 16], 2)                 # 2 and 6 kept rows
    q = dense[0:10].copy()
    ids = np.array([[0], [-1], [1], [-1], [2], [-1], [3], [-1], [4], [-1]])
    res = thin_item(rows, first, q, ids, 2)                       # need = 10 // 2 = 5
    # track 0 is eligible on its own 2 rows; track 1 holds 3 pairs (s = 4, 6, 8) of the 5 it needs
    assert [(t, o, v) for t, o, _, v in res] == [(0, 0, 2)]
    assert res[0][2] == score_run(q[[0, 2]], rows[0:2])
    res = thin_item(rows, first, q, ids, 2, min_overlap=6)        # need = 3
    assert [(t, o, v) for t, o, _, v in res] == [(0, 0, 2), (1, -4, 3)]


def test_query_shorter_than_the_stride():
    dense = _rows(20, 7)
    rows, first = thin_rows(dense, [0, 20], 5)                    # kept: dense 0, 5, 10, 15
    q = dense[9:12].copy()                                        # s = 1 sits on kept row 2
    res = thin_item(rows, first, q, np.array([[-1], [2], [-1]]), 5)
    assert [(t, o, v) for t, o, _, v in res] == [(0, 9, 1)]       # need = max(1, 3 // 5) = 1
    assert res[0][2] == score_run(q[1:2], rows[2:3])
    # a query that lands on no kept row finds nothing to vote for; a hit on the row before it names another alignment
    res = thin_item(rows, first, dense[11:14].copy(), np.array([[2], [-1], [-1]]), 5)
    assert [(t, o, v) for t, o, _, v in res] == [(0, 10, 1)]


def test_equal_scores_smaller_offset_then_smaller_track():
    base = _rows(2, 8)
    rows = np.concatenate([base, base, base, base])               # kept rows: two tracks, each holds base twice
    first = np.array([0, 4, 8])
    q = _rows(4, 9)
    q[[0, 2]] = base                                              # D = 2: query rows 0 and 2 pair with consecutive rows
    ids = np.array([[0, 2, 4, 6], [-1] * 4, [1, 3, 5, 7], [-1] * 4])
    res = thin_item(rows, first, q, ids, 2, top=5)
    assert [(t, o) for t, o, _, _ in res] == [(0, 0), (1, 0)]
    assert res[0][2] == res[1][2] == score_run(base, base)


# ---- the library ----------------------------------------------------------------------------------------------------
def _tiny_model():
    from grafp_amd.train import build_model
    torch.manual_seed(0)
    return build_model(load_config())


def _cpu_lib(model):
    rows = torch.from_numpy(_rows(14, 13))
    return library.FingerprintLibrary(model, load_config(), rows, [0, 0, 7, 8, 14], ["a", "b", "c", "d"],
                                      precision="f32", device="cpu")


def test_thin_selects_rows_and_rebuilds_the_table():
    model = _tiny_model()
    lib = _cpu_lib(model)
    assert lib.row_stride == 1
    thin = lib.thin(3)
    want_rows, want_first = thin_rows(lib.rows().numpy(), lib.first, 3)
    assert thin.row_stride == 3 and thin.first.tolist() == want_first.tolist() == [0, 0, 3, 4, 6]
    assert np.array_equal(thin.rows().numpy(), want_rows) and thin.names == lib.names and thin.precision == "f32"
    assert lib.n_rows == 14 and lib.row_stride == 1 and lib.first.tolist() == [0, 0, 7, 8, 14]      # the source stays
    assert lib.thin(1).first.tolist() == lib.first.tolist()
    with pytest.raises(ValueError, match="row_stride"):
        lib.thin(33)
    with pytest.raises(ValueError, match="row_stride"):
        lib.thin(0)
    with pytest.raises(NotImplementedError, match="row_stride"):
        thin.thin(2)


def test_files_of_a_thinned_library_round_trip(tmp_path):
    model = _tiny_model()
    lib = _cpu_lib(model)
    thin = lib.thin(5)
    thin.save(str(tmp_path / "thin"))
    lib.save(str(tmp_path / "dense"))
    files = ["library.json", "library.mm", "library_shape.npy", "library_tracks.npy"]
    assert sorted(os.listdir(tmp_path / "thin")) == files and sorted(os.listdir(tmp_path / "dense")) == files
    meta = json.load(open(tmp_path / "thin" / "library.json"))
    assert meta["format"] == 3 and meta["row_stride"] == 5 and meta["n_rows"] == thin.n_rows
    dense_meta = json.load(open(tmp_path / "dense" / "library.json"))
    assert dense_meta["format"] == 1 and "row_stride" not in dense_meta
    assert list(dense_meta) == ["format", "names", "settings", "precision", "model_digest", "n_rows", "n_tracks"]
    back = library.FingerprintLibrary.load(str(tmp_path / "thin"), model)
    assert back.row_stride == 5 and back.first.tolist() == thin.first.tolist() and torch.equal(back.rows(), thin.rows())
    assert back.names == thin.names and back.settings == thin.settings
    assert library.FingerprintLibrary.load(str(tmp_path / "dense"), model).row_stride == 1       # a format-1 file
    meta["format"] = 4
    json.dump(meta, open(tmp_path / "thin" / "library.json", "w"))
    with pytest.raises(ValueError, match="format 4"):
        library.FingerprintLibrary.load(str(tmp_path / "thin"), model)


def test_a_thinned_library_refuses_what_needs_every_row():
    model = _tiny_model()
    thin = _cpu_lib(model).thin(2)
    with pytest.raises(NotImplementedError, match="row_stride"):
        thin.compress()
    with pytest.raises(NotImplementedError, match="row_stride"):
        thin.self_matches()
    with pytest.raises(NotImplementedError, match="row_stride"):
        thin.match(np.zeros(16000, np.float32))
    with pytest.raises(NotImplementedError, match="row_stride"):
        library.FingerprintLibrary.build(model, [], load_config(), index="ivfpq", row_stride=2)
    with pytest.raises(ValueError, match="row_stride"):
        library.FingerprintLibrary.build(model, [], load_config(), row_stride=33)


def test_identify_thin_op_refusals_without_a_gpu():
    rows = torch.zeros(8, 128)
    q = torch.zeros(300, 128)
    first = torch.tensor([0, 8])
    ids = torch.zeros(300, 4, dtype=torch.int64)
    one = torch.zeros(1, dtype=torch.int64)
    two = torch.tensor([2], dtype=torch.int32)
    with pytest.raises(ValueError, match="256 segments"):
        ops.identify_thin(rows, first, q, ids, one, torch.tensor([257], dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="k=33"):
        ops.identify_thin(rows, first, q, torch.zeros(300, 33, dtype=torch.int64), one, two, 2)
    with pytest.raises(ValueError, match="hits per item"):
        ops.identify_thin(rows, first, q, torch.zeros(300, 32, dtype=torch.int64), one, two, 2, max_len=257)
    with pytest.raises(ValueError, match="never decrease"):
        ops.identify_thin(rows, torch.tensor([0, 5, 3, 8]), q, ids, one, two, 2)
    with pytest.raises(ValueError, match="outside q_rows"):
        ops.identify_thin(rows, first, q, ids, torch.tensor([299]), two, 2)
    with pytest.raises(ValueError, match="top"):
        ops.identify_thin(rows, first, q, ids, one, two, 2, top=65)
    with pytest.raises(ValueError, match="min_overlap"):
        ops.identify_thin(rows, first, q, ids, one, two, 2, min_overlap=0)
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match=r"row_stride=.* not in \[1, 32\]"):
            ops.identify_thin(rows, first, q, ids, one, two, bad)
    # n * D + 255 must stay below 2^32 (only the row count is read before the refusal: no such array exists)
    huge = torch.empty((1 << 27, 128), device="meta")
    with pytest.raises(ValueError, match="2\\^32"):
        ops.identify_thin(huge, torch.tensor([0, 1 << 27]), q, ids, one, two, 32)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.identify_thin(rows, first, q, ids, one, two, 2)


# ---- the C ABI entry and the shipped object ---------------------------------------------------------------------
def test_abi_entry_follows_the_conventions():
    from test_abi import _ctype_of, _declared
    from grafp_amd import _lib
    d = _declared()
    ret, args = d["grafp_identify_thin_f32"]
    assert ret == "int" and args[-1].startswith("grafp_stream_t")
    dense = d["grafp_identify_f32"][1]
    assert [a for a in args if a != "int row_stride"] == dense and args.index("int row_stride") == 4
    res, argtypes = _lib.SIGNATURES["grafp_identify_thin_f32"]
    assert res is ctypes.c_int and [_ctype_of(a) for a in args] == list(argtypes)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "grafp_identify_thin_f32")


def test_abi_entry_refuses_out_of_range_launches_without_a_gpu():
    from grafp_amd._lib import lib
    # never dereferenced: every call below fails an argument check before anything is launched (no call here may pass
    # them -- this file also runs on machines with a GPU)
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(10)]

    def call(max_len, k, top=5, n=100, stride=2):
        return lib.grafp_identify_thin_f32(fake[0], n, fake[1], 2, stride, fake[2], 1000, fake[3], k, fake[4], fake[5],
                                           4, max_len, top, 0, fake[6], fake[7], fake[8], fake[9], None)
    assert call(257, 4) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(8, 33) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(205, 40) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(8, 4, top=65) == -1 and b"top" in lib.grafp_last_error()
    assert call(8, 4, stride=0) == -1 and b"row_stride" in lib.grafp_last_error()
    assert call(8, 4, stride=33) == -1 and b"row_stride" in lib.grafp_last_error()
    assert call(8, 4, n=1 << 27, stride=32) == -1 and b"2^32" in lib.grafp_last_error()
    assert call(8, 4, n=(1 << 32) // 5, stride=5) == -1 and b"2^32" in lib.grafp_last_error()
    assert lib.grafp_identify_thin_f32(None, 100, fake[1], 2, 2, fake[2], 1000, fake[3], 4, fake[4], fake[5], 4, 8, 5,
                                       0, fake[6], fake[7], fake[8], fake[9], None) == -1
    assert b"null pointer" in lib.grafp_last_error()


def test_identify_thin_kernels_have_no_packed_f32_instructions():
    """The shipped object's own command (make -n), compiled to device assembly: both query-row plans are there and
    neither holds a packed-f32 instruction."""
    asm = shipped_asm("identify_thin")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert sum("identify_thin_kernel" in k for k in kernels) == 2 and len(kernels) == 2
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm


def test_build_takes_a_row_stride_on_the_command_line(capsys):
    from grafp_amd import identify
    with pytest.raises(SystemExit) as e:
        identify.main(["build", "--help"])
    assert e.value.code == 0
    assert "--row-stride" in capsys.readouterr().out
