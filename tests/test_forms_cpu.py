"""The storage forms of a FingerprintLibrary (grafp_amd/_forms.py: FlatForm with its row_stride, HalfForm, CompactForm) and
the one base of ops.FlatL2Index and ops.HalfL2Index: each form launches its own ops on the library's stored tensors and
no sibling's, appended chunks are concatenated once into the form's dtypes, a library without rows has the form's empty
tensors, and save -> load -> save writes the same files.  On the CPU with the ops swapped for fakes; one GPU test at the
end holds the sharing of the stored tensor with the index and the byte counts."""
import os

import numpy as np
import pytest
import torch

from grafp_amd import library, ops
from grafp_amd._forms import CompactForm, HalfForm
from grafp_amd.util import load_config

FORM_NAMES = ("flat", "thin", "half", "compact")
FIRST, TRACK_NAMES, M = [0, 0, 7, 14], ["a", "b", "c"], 16       # 3 tracks, 14 rows, one track without rows
IDENTIFY_OPS = {"flat": "identify", "thin": "identify_thin", "half": "identify_half", "compact": "identify_pq"}
MATCH_OPS = {"flat": "cross_match", "thin": "cross_match", "half": "cross_match_half", "compact": "cross_match_pq"}
ALL_OPS = {"identify", "identify_thin", "identify_half", "identify_pq", "identify_stride", "identify_tempo",
           "identify_tempo_items", "cross_match", "cross_match_half", "cross_match_pq", "cross_match_tempo"}


@pytest.fixture(scope="module")
def model():
    from grafp_amd.train import build_model
    torch.manual_seed(0)
    return build_model(load_config())


def _data(name, n=14, seed=7):
    """The seeded data of n rows in the form that the form's _append* takes."""
    rng = np.random.RandomState(seed)
    rows = torch.from_numpy(rng.randn(n, 128).astype(np.float32))
    if name == "half":
        return (rows.to(torch.bfloat16),)
    if name == "compact":
        return (torch.from_numpy(rng.randint(0, 4, size=n).astype(np.int32)),
                torch.from_numpy(rng.randint(0, 256, size=(n, M)).astype(np.uint8)))
    return (rows,)


def _empty_lib(name, model, device="cpu"):
    """A library of the form without tracks -> (library, its append method)."""
    lib = library.FingerprintLibrary(model, load_config(), None, None, precision="f32", device=device,
                                     row_stride=3 if name == "thin" else 1)
    if name == "half":                                               # (as build(index="half") starts)
        lib._form = HalfForm(lib.device)
    if name == "compact":
        rng = np.random.RandomState(3)
        lib._set_quantiser({"centroids": torch.from_numpy(rng.randn(4, 128).astype(np.float32)),
                            "codebooks": torch.from_numpy(rng.randn(M, 256, 128 // M).astype(np.float32))}, 3)
    return lib, {"half": lib._append_half, "compact": lib._append_codes}.get(name, lib._append)


def _lib(name, model):
    lib, append = _empty_lib(name, model)
    append(*_data(name), FIRST, TRACK_NAMES)
    return lib


def _only(monkeypatch, *allowed):
    """Every identify and match op but `allowed` fails; those record their arguments -> the record."""
    seen = []
    for op in ALL_OPS - set(allowed):
        monkeypatch.setattr(ops, op, lambda *a, _op=op, **k: pytest.fail(f"ops.{_op} was launched"))
    for op in allowed:
        monkeypatch.setattr(ops, op, lambda *a, _op=op, **k: seen.append((_op, a, k)) or _op)
    return seen


ID_ARGS = (torch.zeros(3, 128), torch.zeros((3, 2), dtype=torch.int64), np.zeros(1, np.int64), np.full(1, 3, np.int32), 5,
           None, 3)
ID_KW = dict(top=5, min_overlap=None, max_len=3)
MATCH_KW = dict(top=8, min_votes=4, min_overlap=1)


def _match_args(nums=None):
    return torch.zeros(3, 128), torch.tensor([0, 3]), torch.zeros((3, 2), dtype=torch.int64), nums, MATCH_KW


# ---- routing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORM_NAMES)
def test_each_form_launches_its_own_ops_on_the_stored_tensors(name, model, monkeypatch):
    lib = _lib(name, model)
    stored = lib._stored()
    seen, m_args = _only(monkeypatch, IDENTIFY_OPS[name], MATCH_OPS[name]), _match_args()
    assert lib._identify_lists(*ID_ARGS) == IDENTIFY_OPS[name] and lib._match_launch(*m_args) == MATCH_OPS[name]
    (id_op, a, k), (m_op, b, kb) = seen
    assert (id_op, m_op) == (IDENTIFY_OPS[name], MATCH_OPS[name]) and k == ID_KW and kb == MATCH_KW
    head = len(stored)
    assert all(x is y for x, y in zip(a[:head], stored)) and all(x is y for x, y in zip(b[:head], stored))
    if name == "compact":                                            # the codes, then the quantiser, then the tail
        quant = lib.quantiser()
        assert head == 2 and a[2] is quant["centroids"] and a[3] is quant["codebooks"] and len(a) == 9
        assert b[2] is quant["centroids"] and b[3] is quant["codebooks"] and len(b) == 8
    else:
        assert head == 1 and len(a) == (7 if name == "thin" else 6) and len(b) == 5
        assert name != "thin" or a[6] == 3                           # the stride, after the tail
    skip = head + (2 if name == "compact" else 0)                    # then the track table and the call's own tensors
    assert torch.equal(a[skip], torch.from_numpy(lib.first)) and a[skip + 1] is ID_ARGS[0] and a[skip + 2] is ID_ARGS[1]
    assert torch.equal(b[skip], torch.from_numpy(lib.first)) and all(x is y for x, y in zip(b[skip + 1:], m_args[:3]))


def test_the_flat_form_keeps_its_three_special_routes(model, monkeypatch):
    """query_stride, tempo and per-item tempo stay in the library: flat rows only, the front refused the other forms."""
    lib = _lib("flat", model)
    rows, nums = lib._stored()[0], np.array([250, 256, 262], np.int32)
    ratios = (np.zeros(1, np.int64), np.full(1, 2, np.int64))
    for op, kw, extra in (("identify_stride", dict(q_stride=2), (2,)), ("identify_tempo", dict(nums=nums), (nums,)),
                          ("identify_tempo_items", dict(nums=nums, item_ratios=ratios), (nums, *ratios))):
        seen = _only(monkeypatch, op)
        assert lib._identify_lists(*ID_ARGS, **kw) == op
        (_, a, k), = seen
        assert a[0] is rows and len(a) == 6 + len(extra) and all(x is y for x, y in zip(a[6:], extra)) and k == ID_KW
        monkeypatch.undo()
    seen = _only(monkeypatch, "cross_match_tempo")
    assert lib._match_launch(*_match_args(nums)) == "cross_match_tempo"
    (_, b, kb), = seen
    assert b[0] is rows and len(b) == 6 and b[5] is nums and kb == MATCH_KW


# ---- append and concatenate ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORM_NAMES)
def test_appended_chunks_are_concatenated_once_in_the_forms_dtypes(name, model):
    lib, append = _empty_lib(name, model)
    empty = lib._stored()
    want = {"flat": [((0, 128), torch.float32)], "thin": [((0, 128), torch.float32)],
            "half": [((0, 128), torch.bfloat16)], "compact": [((0,), torch.int32), ((0, M), torch.uint8)]}[name]
    assert [(tuple(t.shape), t.dtype) for t in empty] == want and lib._stored() is empty
    assert (lib.is_half, lib.is_compact, lib.row_stride) == (name == "half", name == "compact", 3 if name == "thin" else 1)
    one, two = _data(name, 9, seed=1), _data(name, 5, seed=2)
    append(*one, [0, 0, 9], ["a", "b"])
    append(*two, [0, 5], ["c"])
    assert len(lib._chunks) == 2
    stored = lib._stored()
    assert lib._stored() is stored and len(lib._chunks) == 1 and lib._chunks[0] is stored
    assert [t.dtype for t in stored] == [d for _, d in want]
    assert all(torch.equal(s, torch.cat([x, y])) for s, x, y in zip(stored, one, two))
    assert lib.first.tolist() == [0, 0, 9, 14] and lib.names == ["a", "b", "c"] and lib.n_rows == 14
    own = {"flat": 14 * 512, "thin": 14 * 512, "half": 14 * 256, "compact": 14 * (M + 4) + 4 * 512 + M * 256 * 8 * 4}
    assert lib.nbytes == own[name]                                   # a CPU device: the form's own tensors only


# ---- files --------------------------------------------------------------------------------------------------------------
def _same_files(a, b):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in os.listdir(a):
        if f.endswith(".npz"):                                       # (a zip container carries timestamps)
            with np.load(os.path.join(a, f)) as x, np.load(os.path.join(b, f)) as y:
                assert sorted(x.files) == sorted(y.files)
                assert all(x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k]) for k in x.files)
        else:
            assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.mark.parametrize("name", FORM_NAMES)
def test_save_load_save_writes_the_same_files(name, model, tmp_path):
    lib = _lib(name, model)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    lib.save(a)
    files = {"flat": ["library.mm", "library_shape.npy"], "thin": ["library.mm", "library_shape.npy"],
             "half": ["library_half.npy"], "compact": ["library_codes.npy", "library_lists.npy", "library_pq.npz"]}[name]
    assert sorted(os.listdir(a)) == sorted(files + ["library.json", "library_tracks.npy"])
    back = library.FingerprintLibrary.load(a, model)
    assert type(back._form) is type(lib._form) and back.row_stride == lib.row_stride and back.nbytes == lib.nbytes
    assert all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(back._stored(), lib._stored()))
    assert back.first.tolist() == FIRST and back.names == TRACK_NAMES
    back.save(b)
    _same_files(a, b)


# ---- the one base of the two exact indexes ------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["FlatL2Index", "HalfL2Index"])
def test_the_exact_indexes_share_their_bookkeeping(cls, monkeypatch):
    calls = {"norm": 0, "bf16": 0, "search": []}

    def norm(db):
        calls["norm"] += 1
        return db.float().pow(2).sum(1)

    def to_bf16(db):
        calls["bf16"] += 1
        return db.to(torch.bfloat16)

    def search(db, sq, q, k, id_base=0, db_bf16=None):
        calls["search"].append((db, sq, q, db_bf16))
        return torch.zeros((q.shape[0], k)), torch.full((q.shape[0], k), id_base, dtype=torch.int64)

    half = cls == "HalfL2Index"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(ops, "_require_gpu", lambda *t: None)
    monkeypatch.setattr(ops, "row_sqnorm_half" if half else "row_sqnorm", norm)
    monkeypatch.setattr(ops, "row_sqnorm" if half else "row_sqnorm_half", lambda db: pytest.fail("the wrong norm op"))
    monkeypatch.setattr(ops, "rows_to_bf16", lambda db: pytest.fail("a half index copies nothing") if half else to_bf16(db))
    monkeypatch.setattr(ops, "search_l2_half" if half else "search_l2", search)
    monkeypatch.setattr(ops, "search_l2" if half else "search_l2_half", lambda *a, **k: pytest.fail("the wrong search op"))
    index = getattr(ops, cls)(d=128, device="cpu", id_base=5)
    # the empty index: inf / -1 of shape (nq, k), numpy for numpy
    D, I = index.search(np.zeros((3, 128), np.float32), 4)
    assert isinstance(D, np.ndarray) and D.shape == (3, 4) and np.isinf(D).all() and D.dtype == np.float32
    assert isinstance(I, np.ndarray) and I.shape == (3, 4) and (I == -1).all() and I.dtype == np.int64
    D, I = index.search(torch.zeros(2, 128), 1)
    assert isinstance(D, torch.Tensor) and tuple(I.shape) == (2, 1) and index.held_tensors() == [] and not calls["search"]
    # two add calls: one concatenation, one norm pass, one chunk kept
    dtype = torch.bfloat16 if half else torch.float32
    x1, x2 = torch.ones((5, 128), dtype=dtype), torch.full((3, 128), 2.0, dtype=dtype)
    index.add(x1)
    index.add(x2 if half else x2.numpy())
    assert index.ntotal == 8 and len(index._chunks) == 2
    q = torch.zeros(2, 128)
    D, I = index.search(q, 3)
    index.search(q.numpy().reshape(-1), 3)                             # anything that reshapes to (nq, d)
    db, sq = index._materialise()
    assert calls["norm"] == 1 and calls["bf16"] == (0 if half else 1) and len(index._chunks) == 1 and index._chunks[0] is db
    assert torch.equal(db, torch.cat([x1, x2])) and db.dtype == dtype and torch.equal(sq, torch.tensor([128.0] * 5 + [512.0] * 3))
    assert all(c[0] is db and c[1] is sq and tuple(c[2].shape) == (2, 128) for c in calls["search"]) and len(calls["search"]) == 2
    assert calls["search"][0][3] is index._bf16 and (index._bf16 is None) == half
    assert isinstance(D, torch.Tensor) and (I == 5).all()
    held = index.held_tensors()
    assert len(held) == (2 if half else 3) and held[0] is db and held[1] is sq
    assert sum(t.numel() * t.element_size() for t in held) == (260 if half else 772) * 8
    if half:
        assert index.nbytes == 260 * 8 and index.half_rows() is db and not hasattr(index, "rows")
    else:
        assert index.rows() is db and index.nprobe == 1
        plain = ops.FlatL2Index(device="cpu", prefilter=False)
        plain.add(x1)
        assert len(plain.held_tensors()) == 2 and plain._bf16 is None and calls["bf16"] == 1
    # a later add is concatenated at the next use
    index.add(x1)
    assert index._materialise()[0].shape[0] == 13 and calls["norm"] == (2 if half else 3) and len(index._chunks) == 1


# ---- on the device: one rows tensor, shared with the index ---------------------------------------------------------------
@pytest.mark.gpu
def test_each_form_shares_its_stored_tensor_with_its_index():
    """3 tracks and 40 rows of the same seeded unit rows as flat, thinned (D = 2), half and compact (M = 16, nlist = 4):
    the index is made once, it searches the library's own tensor, and nbytes is the storage-deduplicated sum of the form's
    tensors and the index's -- 772 bytes a row (flat, thinned), 260 (half), at most 2 M + 24 and the quantiser (compact)."""
    dev, cfg = torch.device("cuda:0"), load_config()
    rng = np.random.RandomState(11)
    rows = torch.from_numpy(rng.randn(40, 128).astype(np.float32))
    rows = (rows / rows.norm(dim=1, keepdim=True)).to(dev)
    first = [0, 13, 26, 40]
    flat = library.FingerprintLibrary(None, cfg, rows, first, precision="f32", device=dev)
    quantiser = {"centroids": torch.from_numpy(rng.randn(4, 128).astype(np.float32) * 0.1),
                 "codebooks": torch.from_numpy(rng.randn(M, 256, 128 // M).astype(np.float32) * 0.1)}
    list_id, codes = CompactForm(dev, quantiser, 4).encode(rows)
    libs = {"flat": flat, "thin": flat.thin(2), "half": flat.halve(),
            "compact": library.FingerprintLibrary.from_codes(None, cfg, quantiser, list_id, codes, first, precision="f32",
                                                             device=dev, nprobe=4)}
    assert libs["thin"].n_rows == 7 + 7 + 7 and libs["thin"].row_stride == 2

    def storage_bytes(tensors):
        return sum({t.untyped_storage().data_ptr(): t.untyped_storage().nbytes() for t in tensors}.values())

    for name, lib in libs.items():
        n, stored = lib.n_rows, lib._stored()
        own = lib._form.held_tensors(stored)
        assert lib._index is None
        index = lib.index
        assert lib.index is index and lib._stored() is stored
        total = lib.nbytes
        assert lib.index is index and lib.nbytes == total                                   # made once, reused
        assert total == storage_bytes(own + index.held_tensors())
        if name == "compact":
            quant = sum(v.numel() * 4 for v in lib.quantiser().values())
            assert total <= n * (2 * M + 24) + quant
            assert index._codes[0].data_ptr() == stored[1].data_ptr()                       # the row-order codes
            assert index.centroids.data_ptr() == lib.quantiser()["centroids"].data_ptr()
        else:
            assert total == n * (260 if name == "half" else 772)
            assert index._materialise()[0].data_ptr() == stored[0].data_ptr()
        ids = lib._search_rows(rows[:5], 3)
        assert tuple(ids.shape) == (5, 3) and lib.index is index
    assert torch.equal(libs["flat"]._search_rows(rows[:5], 1)[:, 0].cpu(), torch.arange(5))
