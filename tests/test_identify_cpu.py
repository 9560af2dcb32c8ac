"""CPU tests of track-aware identification (csrc/identify.hip, ops.identify, grafp_amd/library.py): the numpy
restatement on hand-built cases, the host bookkeeping of the library, its files, the refusal paths, the C ABI entry and
the shipped assembly.  No GPU call is made."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _identify_ref import identify_item, identify_ref, score_run
from grafp_amd import library, ops
from grafp_amd.util import load_config


def _rows(n, seed):
    """Dyadic rows (multiples of 2^-8 in [-1/8, 1/8)): every product and partial sum is exact in f32."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-32, 32, size=(n, 128)) / 256.0).astype(np.float32)


def test_score_run_is_the_mean_dot_product_on_exact_inputs():
    q, r = _rows(5, 1), _rows(5, 2)
    assert score_run(q, r) == np.float32((q.astype(np.float64) * r).sum() / 5)


def test_run_across_a_track_boundary_is_rejected_or_clipped():
    first = np.array([0, 10, 20])
    rows = _rows(20, 3)
    q = rows[7:11].copy()                      # rows 7..10: the last 3 of track 0 + the first of track 1
    ids = np.array([[7], [8], [9], [10]])
    # default (min_overlap = ql): a = 7 lies in track 0 for s < 3 only, track 1 holds only s = 3 -> neither eligible
    assert identify_item(rows, first, q, ids) == []
    # min_overlap 3: track 0 is scored on its own 3 rows, never on row 10
    res = identify_item(rows, first, q, ids, min_overlap=3)
    assert [(t, o, v) for t, o, _, v in res] == [(0, 7, 3)]
    assert res[0][2] == score_run(q[:3], rows[7:10])


def test_track_shorter_than_the_query():
    first = np.array([0, 3, 13])
    rows = _rows(13, 4)
    q = np.concatenate([_rows(1, 5), rows[0:3], _rows(1, 6)])     # the 3-row track sits at s = 1..3 of a 5-row query
    ids = np.array([[-1], [0], [1], [2], [-1]])
    res = identify_item(rows, first, q, ids)
    assert [(t, o, v) for t, o, _, v in res] == [(0, -1, 3)]
    assert res[0][2] == score_run(q[1:4], rows[0:3])


def test_duplicate_hits_count_as_votes_and_minus_one_is_no_hit():
    first = np.array([0, 8, 16])
    rows = _rows(16, 7)
    q = rows[9:12].copy()
    ids = np.array([[9, 9, -1], [10, -1, 3], [11, 12, -1]])     # (t=1, a=9): 4 hits; row 12 at s=2 -> a=10; row 3 -> a=2
    res = identify_item(rows, first, q, ids, top=5)
    assert res[0][:2] == (1, 1) and res[0][3] == 4
    assert {(t, o) for t, o, _, _ in res} == {(1, 1), (0, 2)}   # the second track-1 candidate loses to the first
    empty = identify_item(rows, first, q, np.full((3, 3), -1))
    assert empty == []


def test_equal_scores_smaller_offset_then_smaller_track():
    first = np.array([0, 4, 8, 12])
    base = _rows(2, 8)
    rows = np.concatenate([base, base, base, base, base, base])    # every track holds base twice
    q = base.copy()
    ids = np.array([[0, 2, 4, 8], [1, 3, 5, 9]])
    res = identify_item(rows, first, q, ids, top=5)
    assert [(t, o) for t, o, _, _ in res] == [(0, 0), (1, 0), (2, 0)]
    assert res[0][2] == res[1][2] == res[2][2]


def test_zero_row_tracks():
    first = np.array([0, 0, 5, 5, 5, 9, 9])
    rows = _rows(9, 9)
    q = rows[5:8].copy()
    res = identify_item(rows, first, q, np.array([[5], [6], [7]]))
    assert [(t, o, v) for t, o, _, v in res] == [(4, 0, 3)]
    res = identify_item(rows, first, rows[1:4].copy(), np.array([[1], [2], [3]]))
    assert [(t, o) for t, o, _, _ in res] == [(1, 1)]


def test_min_overlap_below_the_query_length_gives_negative_offsets():
    first = np.array([0, 6, 12])
    rows = _rows(12, 10)
    q = np.concatenate([_rows(2, 11), rows[6:9]])                # track 1 starts at query segment 2
    ids = np.array([[-1], [-1], [6], [7], [8]])
    assert identify_item(rows, first, q, ids) == []
    res = identify_item(rows, first, q, ids, min_overlap=3)
    assert [(t, o, v) for t, o, _, v in res] == [(1, -2, 3)]
    assert res[0][2] == score_run(q[2:], rows[6:9])


def test_padding_of_the_batched_restatement():
    first = np.array([0, 4])
    rows = _rows(4, 12)
    tr, off, sc, vo = identify_ref(rows, first, rows, np.array([[0], [1], [2], [3]]), [0, 2], [2, 0], top=3)
    assert tr.tolist() == [[0, -1, -1], [-1, -1, -1]]
    assert off[0, 0] == 0 and off[0, 1] == np.iinfo(np.int32).min and np.isneginf(sc[1]).all() and vo[1].sum() == 0


# ---- host bookkeeping -------------------------------------------------------------------------------------------
def test_segment_counts_match_the_oracle_unfold():
    from oracle import model as om
    cfg = load_config()
    step = int(cfg["n_frames"] * (1 - cfg["overlap"]))
    for T in (0, 700, 512 * 30, 512 * 31 - 1, 512 * 31, 16000, 48000, 48001, 160000):
        if T == 0:
            assert library.n_segments(0, cfg) == 0
            continue
        frames = om.logmel(torch.randn(1, T) * 0.1, cfg).shape[-1]
        want = 0 if frames < cfg["n_frames"] else torch.zeros(frames, 1).unfold(0, cfg["n_frames"], step).shape[0]
        assert library.n_segments(T, cfg) == want, T


def test_offset_seconds_formula():
    cfg = load_config()
    assert library.segment_step(cfg) == 3
    assert library.segment_seconds(cfg) == 3 * 512 / 16000
    cfg2 = dict(cfg, overlap=0.5, hop_len=256, fs=8000)
    assert library.segment_seconds(cfg2) == 16 * 256 / 8000


def test_window_items():
    cfg = load_config()
    fs = cfg["fs"]
    n = 10 * fs
    total = library.n_segments(n, cfg)
    starts, rows, lens = library.window_items(total, n, cfg, window_s=3.0, hop_s=1.0)
    assert starts.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    per = library.n_segments(3 * fs, cfg)
    seg_hop = 3 * 512
    for s, r, l in zip(starts, rows, lens):
        assert r * seg_hop >= s * fs and (r - 1) * seg_hop < s * fs            # the first segment at or after the start
        assert l == min(per, total - r)
    assert lens[0] == per and (rows + lens <= total).all()
    # shorter than one window: one item with what there is; shorter than one segment: an empty item
    s1, r1, l1 = library.window_items(library.n_segments(fs, cfg), fs, cfg, 3.0, 1.0)
    assert s1.tolist() == [0.0] and r1.tolist() == [0] and l1.tolist() == [library.n_segments(fs, cfg)]
    assert library.window_items(0, 100, cfg)[2].tolist() == [0]


def _tiny_model():
    from grafp_amd.train import build_model
    torch.manual_seed(0)
    return build_model(load_config())


def test_library_tables_save_load_and_digest_refusal(tmp_path):
    cfg = load_config()
    model = _tiny_model()
    rows = torch.from_numpy(_rows(9, 13))
    lib = library.FingerprintLibrary(model, cfg, rows, [0, 4, 4, 9], ["a", "b", "c"], precision="f32", device="cpu")
    assert lib.n_tracks == 3 and lib.n_rows == 9 and lib.step == 3
    lib._append(torch.from_numpy(_rows(2, 14)), [0, 2], ["d"])
    assert lib.first.tolist() == [0, 4, 4, 9, 11] and lib.names == ["a", "b", "c", "d"]
    lib.save(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["library.json", "library.mm", "library_shape.npy", "library_tracks.npy"]
    from grafp_amd.eval import load_memmap_data
    mm, shape = load_memmap_data(str(tmp_path), "library", display=False)
    assert tuple(shape) == (11, 128) and np.array_equal(np.asarray(mm), lib.rows().numpy())
    meta = json.load(open(tmp_path / "library.json"))
    assert meta["names"] == lib.names and meta["precision"] == "f32" and meta["settings"]["overlap"] == cfg["overlap"]
    back = library.FingerprintLibrary.load(str(tmp_path), model)
    assert back.first.tolist() == lib.first.tolist() and torch.equal(back.rows(), lib.rows())
    assert back.names == lib.names and back.settings == lib.settings and back.precision == "f32"
    other = _tiny_model()
    with torch.no_grad():
        next(other.parameters()).add_(1.0)
    with pytest.raises(ValueError, match="another model"):
        library.FingerprintLibrary.load(str(tmp_path), other)
    assert library.FingerprintLibrary.load(str(tmp_path), other, force=True).n_rows == 11


def test_library_refuses_bad_tables():
    model = _tiny_model()
    rows = torch.from_numpy(_rows(4, 15))
    for bad in ([0, 3, 2, 4], [1, 4], [0, 3], [0]):
        with pytest.raises(ValueError, match="track table"):
            library.FingerprintLibrary(model, load_config(), rows, bad, device="cpu")
    with pytest.raises(ValueError, match="names"):
        library.FingerprintLibrary(model, load_config(), rows, [0, 4], ["a", "b"], device="cpu")


def test_identify_op_refusals_without_a_gpu():
    rows = torch.zeros(8, 128)
    q = torch.zeros(300, 128)
    first = torch.tensor([0, 8])
    ids = torch.zeros(300, 4, dtype=torch.int64)
    one = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="256 segments"):
        ops.identify(rows, first, q, ids, one, torch.tensor([257], dtype=torch.int32))
    with pytest.raises(ValueError, match="k=33"):
        ops.identify(rows, first, q, torch.zeros(300, 33, dtype=torch.int64), one, torch.tensor([2], dtype=torch.int32))
    with pytest.raises(ValueError, match="hits per item"):
        ops.identify(rows, first, q, torch.zeros(300, 32, dtype=torch.int64), one, torch.tensor([2], dtype=torch.int32),
                     max_len=257)
    with pytest.raises(ValueError, match="never decrease"):
        ops.identify(rows, torch.tensor([0, 5, 3, 8]), q, ids, one, torch.tensor([2], dtype=torch.int32))
    with pytest.raises(ValueError, match="outside q_rows"):
        ops.identify(rows, first, q, ids, torch.tensor([299]), torch.tensor([2], dtype=torch.int32))
    with pytest.raises(ValueError, match="top"):
        ops.identify(rows, first, q, ids, one, torch.tensor([2], dtype=torch.int32), top=65)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.identify(rows, first, q, ids, one, torch.tensor([2], dtype=torch.int32))


# what each of the four identify ops takes besides the shared arguments (n library rows)
_IDENTIFY_OPS = {
    "identify": lambda n: dict(index_rows=torch.zeros(n, 128)),
    "identify_thin": lambda n: dict(index_rows=torch.zeros(n, 128), row_stride=2),
    "identify_tempo": lambda n: dict(index_rows=torch.zeros(n, 128), ratio_num=[240, 256]),
    "identify_pq": lambda n: dict(list_id=torch.zeros(n, dtype=torch.int32), codes=torch.zeros((n, 64), dtype=torch.uint8),
                                  centroids=torch.zeros(3, 128), codebooks=torch.zeros(64, 256, 2)),
}
# (case, changed arguments, k, the fragment every op's message holds, whether the message is the op's own and so starts
# with its name -- the track table's comes from check_track_table and the device refusal from _require_gpu)
_SHARED_REFUSALS = [
    ("top_0", dict(top=0), 4, "top=0 not in [1, 64]", True),
    ("top_65", dict(top=65), 4, "top=65 not in [1, 64]", True),
    ("k_33", dict(), 33, "k=33 hits per segment exceeds 32", True),
    ("min_overlap_0", dict(min_overlap=0), 4, "min_overlap must be at least 1 segment", True),
    ("item_of_257", dict(item_len=torch.tensor([257], dtype=torch.int32)), 4,
     "items of 257 segments with k=4 exceed 256 segments or 8192 hits per item", True),
    ("max_len_257", dict(max_len=257), 4, "items of 257 segments with k=4 exceed 256 segments or 8192 hits per item", True),
    ("256_x_32_accepted", dict(item_len=torch.tensor([256], dtype=torch.int32)), 32, "no CPU", False),
    ("256_x_32_accepted_max_len", dict(max_len=256), 32, "no CPU", False),
    ("129_x_64_refused_on_k", dict(item_len=torch.tensor([129], dtype=torch.int32)), 64,
     "k=64 hits per segment exceeds 32", True),
    ("decreasing_table", dict(track_first_row=torch.tensor([0, 5, 3, 8])), 4, "never decrease", False),
    ("item_outside_q_rows", dict(item_row=torch.tensor([299])), 4, "an item reaches outside q_rows", True),
    ("valid", dict(), 4, "no CPU", False),
]


@pytest.mark.parametrize("case,changed,k,fragment,named", _SHARED_REFUSALS, ids=[c[0] for c in _SHARED_REFUSALS])
@pytest.mark.parametrize("op", sorted(_IDENTIFY_OPS))
def test_identify_ops_share_their_refusals(op, case, changed, k, fragment, named):
    """The checks the four identify ops share refuse the same arguments with the same words, each under its own name."""
    args = dict(_IDENTIFY_OPS[op](8), track_first_row=torch.tensor([0, 8]), q_rows=torch.zeros(300, 128),
                topk_ids=torch.zeros(300, k, dtype=torch.int64), item_row=torch.zeros(1, dtype=torch.int64),
                item_len=torch.tensor([2], dtype=torch.int32))
    args.update(changed)
    with pytest.raises(RuntimeError if fragment == "no CPU" else ValueError) as e:
        getattr(ops, op)(**args)
    message = str(e.value)
    assert fragment in message
    if named:
        assert message.startswith(op + ": ")
    elif case == "decreasing_table":
        assert message.startswith("identify: the track table")


# ---- the C ABI entry and the shipped object ---------------------------------------------------------------------
def test_abi_entry_follows_the_conventions():
    from test_abi import _ctype_of, _declared
    from grafp_amd import _lib
    d = _declared()
    ret, args = d["grafp_identify_f32"]
    assert ret == "int" and args[-1].startswith("grafp_stream_t")
    res, argtypes = _lib.SIGNATURES["grafp_identify_f32"]
    assert res is ctypes.c_int and [_ctype_of(a) for a in args] == list(argtypes)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "grafp_identify_f32")


def test_abi_entry_refuses_out_of_range_launches_without_a_gpu():
    from grafp_amd._lib import lib
    # never dereferenced: every call below fails an argument check before anything is launched (no call here may pass
    # them -- this file also runs on machines with a GPU)
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(10)]

    def call(max_len, k, top=5, n=100):
        return lib.grafp_identify_f32(fake[0], n, fake[1], 2, fake[2], 1000, fake[3], k, fake[4], fake[5], 4, max_len,
                                      top, 0, fake[6], fake[7], fake[8], fake[9], None)
    assert call(257, 4) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(8, 33) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(205, 40) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(8, 4, top=65) == -1 and b"top" in lib.grafp_last_error()
    assert lib.grafp_identify_f32(None, 100, fake[1], 2, fake[2], 1000, fake[3], 4, fake[4], fake[5], 4, 8, 5, 0,
                                  fake[6], fake[7], fake[8], fake[9], None) == -1
    assert b"null pointer" in lib.grafp_last_error()


def test_identify_kernel_has_no_packed_f32_instructions():
    """The shipped object's own command (make -n), compiled to device assembly: no packed-f32 instruction in
    identify.hip."""
    asm = shipped_asm("identify")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert sum("identify_kernel" in k for k in kernels) == 2
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm


def test_command_line_parses_both_subcommands(capsys):
    from grafp_amd import identify
    for argv in (["--help"], ["build", "--help"], ["query", "--help"]):
        with pytest.raises(SystemExit) as e:
            identify.main(argv)
        assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--source" in out and "--library" in out and "--window" in out
    with pytest.raises(SystemExit) as e:
        identify.main(["query", "--library", "lib"])                 # --ckp and the files are required
    assert e.value.code == 2
