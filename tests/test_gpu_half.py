"""The half form of a fingerprint library on the MI355X (bf16 rows and their norms only).  The contract: with B the bf16
rows and U = B.float() (exact), every half op on B returns the bits of its flat sibling on U -- ops.search_l2_half /
ops.HalfL2Index against ops.FlatL2Index (and oracle.native.flat_search_l2), ops.identify_half against ops.identify (and
tests/_identify_ref.py), ops.cross_match_half against ops.cross_match (and tests/_crossmatch_ref.py) -- and a half
FingerprintLibrary answers identify, identify_windows, timeline, match and StreamMonitor as the flat library over U."""
import json
import os

import numpy as np
import pytest
import torch

from _crossmatch_ref import cross_match_ref
from _half_ref import bf16_bits, round_bf16
from _identify_ref import identify_ref
from _retrieval_case import add_noise, build_case, synth_tracks
from oracle import native as onative
from test_gpu_crossmatch import _case as crossmatch_case
from test_gpu_identify import _dyadic_case
from grafp_amd import ops
from grafp_amd.library import HALF_SCORE_BOUND, FingerprintLibrary
from grafp_amd.monitor import StreamMonitor
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
ID_NAMES = ("track", "offset", "score", "votes")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits_equal(got, want, tag):
    """torch.equal on every output, the f32 ones compared as bits."""
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, j)
        if g.dtype == torch.float32:
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g, w), (tag, j, (g != w).nonzero()[:5].tolist())


# ---- the search -------------------------------------------------------------------------------------------------------
# The query counts at which grafp_knn_search_l2_pre's plan changes (pre_plan in csrc/knn_search.hip): 2 x 2 waves up to 64
# queries and 4 x 1 from 65; two query sets per wave from 1024; three from 1536 (when the padding allows: 1536 itself); the
# two-part scan with the tightening step from 768 queries, but only over at least 4 * 65536 rows -- its own case below.
SEARCH_N = (1, 5, 257, 20011)
SEARCH_NQ = (1, 33, 64, 65, 800, 1100, 1536)


@pytest.fixture(scope="module")
def search_data(dev):
    """Random unit rows X per database size -> (B = rows_to_bf16(X), the flat index over U = B.float(), the half index
    over B, U on the host), and 1536 unit queries, made once."""
    gen = torch.Generator().manual_seed(5)
    q = torch.nn.functional.normalize(torch.randn(max(SEARCH_NQ), 128, generator=gen), dim=1).to(dev)
    data = {}
    for n in SEARCH_N:
        x = torch.nn.functional.normalize(torch.randn(n, 128, generator=gen), dim=1).to(dev)
        b = ops.rows_to_bf16(x)
        u = b.float()
        flat, half = ops.FlatL2Index(device=dev), ops.HalfL2Index(device=dev)
        flat.add(u)
        half.add(b)
        data[n] = (b, flat, half, u.cpu().numpy())
    return q, data


@pytest.mark.parametrize("k", [1, 20])
@pytest.mark.parametrize("n", SEARCH_N)
def test_search_equals_the_flat_index_over_the_widened_rows(dev, search_data, n, k):
    q, data = search_data
    b, flat, half, u_host = data[n]
    assert half.ntotal == n and half.half_rows() is b and half.nbytes == 260 * n and not hasattr(half, "rows")
    assert torch.equal(half._materialise()[1], ops.row_sqnorm(b.float()))          # contract item 2: the same chain
    for nq in SEARCH_NQ:
        d_h, i_h = half.search(q[:nq], k)
        d_f, i_f = flat.search(q[:nq], k)
        assert torch.equal(i_h, i_f), (n, nq, k, (i_h != i_f).nonzero()[:5].tolist())
        assert torch.equal(d_h.view(torch.int32), d_f.view(torch.int32)), (n, nq, k)
        if n < k:                                                    # padding: id -1, distance +inf
            assert (i_h[:, n:] == -1).all() and torch.isinf(d_h[:, n:]).all() and (i_h[:, :n] >= 0).all()
        if n <= 257:
            d_o, i_o = onative.flat_search_l2(u_host, q[:nq].cpu().numpy(), k)
            assert np.array_equal(i_h.cpu().numpy(), i_o) and np.array_equal(d_h.cpu().numpy().view(np.uint32),
                                                                            d_o.view(np.uint32)), (n, nq, k)


def test_search_through_the_two_part_scan(dev):
    """768 queries over 262 144 rows: the first quarter is scanned with the pre-pass bound, the tightening step runs (it
    reads no database row: the half entry launches it with no database) and the rest is scanned with its bound."""
    gen = torch.Generator(device=dev).manual_seed(6)
    x = torch.nn.functional.normalize(torch.randn(262144, 128, generator=gen, device=dev), dim=1)
    q = torch.nn.functional.normalize(torch.randn(768, 128, generator=gen, device=dev), dim=1)
    b = ops.rows_to_bf16(x)
    del x
    u = b.float()
    d_h, i_h = ops.search_l2_half(b, ops.row_sqnorm_half(b), q, 20)
    d_f, i_f = ops.search_l2(u, ops.row_sqnorm(u), q, 20, db_bf16=b)
    assert torch.equal(i_h, i_f) and torch.equal(d_h.view(torch.int32), d_f.view(torch.int32))


def test_search_ties_that_overflow_a_candidate_list(dev):
    """5 000 copies of one bf16-exact row among 1 000 others, that row as the query: every copy is at distance 0, the
    candidate lists overflow and the select kernel rescans every row exactly -- the only route to the rescan in the half
    instantiation.  The answer is the 20 lowest ids at distance 0."""
    gen = torch.Generator().manual_seed(7)
    row = (torch.randint(-16, 16, (128,), generator=gen) / 256.0)
    row = row / 4 + 0.25 * (row == 0)                                # bf16-exact, no zero row
    assert torch.equal(row.to(torch.bfloat16).float(), row)
    others = torch.nn.functional.normalize(torch.randn(1000, 128, generator=gen), dim=1)
    x = torch.cat([row[None].expand(5000, 128), others]).to(dev)
    b = ops.rows_to_bf16(x)
    assert torch.equal(b[:5000].float(), x[:5000])
    half, flat = ops.HalfL2Index(device=dev), ops.FlatL2Index(device=dev)
    half.add(b)
    flat.add(b.float())
    q = torch.cat([row[None], others[:3]]).to(dev)
    d_h, i_h = half.search(q, 20)
    assert i_h[0].tolist() == list(range(20)) and (d_h[0] == 0).all()
    d_f, i_f = flat.search(q, 20)
    assert torch.equal(i_h, i_f) and torch.equal(d_h.view(torch.int32), d_f.view(torch.int32))


# ---- identify_half ------------------------------------------------------------------------------------------------------
def _identify_both(dev, rows, first, q, ids, item_row, item_len, **kw):
    """ops.identify_half on B and ops.identify on U, for dyadic rows (U = rows: they are bf16-exact)."""
    u = _t(dev, rows)
    b = ops.rows_to_bf16(u)
    assert torch.equal(b.float(), u)
    tail = (_t(dev, first), _t(dev, q), _t(dev, ids), _t(dev, item_row), _t(dev, item_len))
    return ops.identify_half(b, *tail, **kw), ops.identify(u, *tail, **kw)


@pytest.mark.parametrize("min_overlap", [None, 1, 3])
def test_identify_half_matches_the_flat_op_and_the_restatement_on_dyadic_inputs(dev, min_overlap):
    """tests/test_gpu_identify.py's dyadic generator (multiples of 2^-8 in [-1/16, 1/16): bf16-exact rows, exact sums, so
    the numpy restatement agrees bit for bit): zero-row tracks, an item of length 0, equal scores, runs across track ends."""
    rows, first, q, ids, item_row, item_len = _dyadic_case(21 + (min_overlap or 0), 96, 40, 6)
    assert item_len[0] == 0 and (np.diff(first) == 0).any()
    got, flat = _identify_both(dev, rows, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap)
    _bits_equal(got, flat, min_overlap)
    want = identify_ref(rows, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap)
    for g, w, name in zip(got, want, ID_NAMES):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, np.argwhere(g != w)[:5])
    assert (got[0][:, 0] >= 0).sum() > 40                            # most items found something
    assert (got[0][0] == -1).all() and torch.isneginf(got[2][0]).all() and (got[3][0] == 0).all()   # the empty item
    again, _ = _identify_both(dev, rows, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap,
                              max_len=int(item_len.max()))            # the asynchronous path
    _bits_equal(again, got, "max_len")


@pytest.mark.parametrize("max_len,k", [(ops.IDENTIFY_MAX_LEN, ops.IDENTIFY_MAX_KEYS // ops.IDENTIFY_MAX_LEN), (128, 32),
                                       (129, 32)])
def test_identify_half_at_the_size_limits_and_on_both_query_row_plans(dev, max_len, k):
    """256 segments at k = 32 (8 192 keys: the limits), and the two shapes next to identify_plan's switch at k = 32: 128
    segments (4 096 slots + the query rows fit the LDS) and 129 (8 192 slots: the query rows are read from global
    memory).  A 5-segment item rides in the same launch."""
    rows, first, _, _, _, _ = _dyadic_case(27, 3, 8, k)
    item_len = np.array([max_len, 5, max_len - 56], np.int32)
    item_row = np.concatenate([[0], np.cumsum(item_len[:-1])]).astype(np.int64)
    nq = int(item_len.sum())
    rng = np.random.RandomState(8)
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = rng.randint(-1, rows.shape[0], size=(nq, k)).astype(np.int64)
    ids[:, min(5, k - 1)] = np.arange(nq) % rows.shape[0]            # long runs of one alignment
    for mo in (None, 1):
        got, flat = _identify_both(dev, rows, first, q, ids, item_row, item_len, top=16, min_overlap=mo)
        _bits_equal(got, flat, (max_len, mo))
        want = identify_ref(rows, first, q, ids, item_row, item_len, top=16, min_overlap=mo)
        for g, w, name in zip(got, want, ID_NAMES):
            assert np.array_equal(g.cpu().numpy(), w), (max_len, mo, name)
    assert (got[0][:, 0] >= 0).all()


# ---- cross_match_half ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_votes,min_overlap", [(4, 1), (1, 1)])
def test_cross_match_half_matches_the_flat_op_and_the_restatement(dev, min_votes, min_overlap):
    """2 000 dyadic (bf16-exact) rows in 9 tracks, one of them empty; sources of 1, 40 and 700 rows with planted copies,
    one across a track end; top 8; min_votes and min_overlap at their defaults and at 1."""
    lib_lens = np.array([300, 150, 0, 400, 250, 200, 350, 100, 250])
    first = np.concatenate([[0], np.cumsum(lib_lens)])
    plants = [(0, 0, int(first[4]) + 7, 1), (1, 2, int(first[1]) + 20, 30), (1, 0, int(first[8]) + 3, 12),
              (2, 10, int(first[3]), 400), (2, 450, int(first[6]) - 20, 60), (2, 600, int(first[7]), 100)]
    _, rows, first, q, src_first, ids = crossmatch_case(31, lib_lens, np.array([1, 40, 700]), 8, plants, p_random=0.1)
    u = _t(dev, rows)
    b = ops.rows_to_bf16(u)
    assert torch.equal(b.float(), u) and rows.shape[0] == 2000
    tail = (_t(dev, first), _t(dev, q), _t(dev, src_first), _t(dev, ids))
    kw = dict(top=8, min_votes=min_votes, min_overlap=min_overlap)
    got, flat = ops.cross_match_half(b, *tail, **kw), ops.cross_match(u, *tail, **kw)
    _bits_equal(got, flat, (min_votes, min_overlap))
    want = cross_match_ref(rows, first, q, src_first, ids, **kw)
    for j, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and np.array_equal(g, w), (j, np.argwhere(g != w)[:5])
    assert {3, 7} <= set(got[0][2].tolist())                          # the 700-row source holds tracks 3 and 7
    if (min_votes, min_overlap) == (4, 1):                           # the defaults are these
        _bits_equal(ops.cross_match_half(b, *tail), got, "defaults")


# ---- the library ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_libs(dev):
    """The untrained model and the 8 synthetic tracks of tests/test_gpu_identify.py's small_lib: the flat library over X,
    H = flat.halve() and F_U, the flat library over U = H.half_rows().float()."""
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    tracks = synth_tracks(8, 84 * SEG_HOP / 16000, 4242, dev)            # 8.06 s: a whole number of segment hops
    names = [f"song{i}" for i in range(8)]
    flat = FingerprintLibrary.build(model, list(tracks), cfg, names=names, max_segments=200)
    half = flat.halve()
    f_u = FingerprintLibrary(model, flat.settings, half.half_rows().float(), flat.first, names)
    return cfg, model, tracks, flat, half, f_u


def _queries(tracks):
    rng = np.random.RandomState(11)
    crops = []
    for i in range(40):
        L = int(rng.randint(3 * 16000, 5 * 16000))
        j = rng.randint(0, (tracks.shape[1] - L) // SEG_HOP + 1)
        crops.append(tracks[i % 8, j * SEG_HOP:j * SEG_HOP + L])
    return crops + [tracks[0, :3000]]                                    # the last: shorter than one segment


def test_halve_keeps_the_tables_and_260_bytes_a_row(small_libs, dev):
    cfg, model, tracks, flat, half, f_u = small_libs
    n = flat.n_rows
    assert half.is_half and not half.is_compact and not flat.is_half and flat.rows().dtype == torch.float32
    assert half.first.tolist() == flat.first.tolist() and half.names == flat.names and half.n_rows == n
    assert torch.equal(half.half_rows(), ops.rows_to_bf16(flat.rows()))
    assert np.array_equal(half.half_rows().float().cpu().numpy(), round_bf16(flat.rows().cpu().numpy()))
    assert half.nbytes == 260 * n and flat.nbytes == 772 * n
    assert isinstance(half.index, ops.HalfL2Index) and half.index.half_rows() is half.half_rows()    # one tensor, shared
    assert half.nbytes == 260 * n                                        # with the index made, still


def test_the_half_library_answers_as_the_flat_library_over_its_rows(small_libs, dev):
    cfg, model, tracks, flat, half, f_u = small_libs
    crops = _queries(tracks)
    res_h, res_u, res_x = half.identify(crops), f_u.identify(crops), flat.identify(crops)
    assert res_h == res_u and res_h[-1] == [] and all(res_h[:-1])
    assert half.identify(crops[0]) == f_u.identify(crops[0])
    assert half.identify(crops, top=3, k_probe=8, min_overlap=5) == f_u.identify(crops, top=3, k_probe=8, min_overlap=5)
    agree = sum(a[0]["track"] == b[0]["track"] and a[0]["offset"] == b[0]["offset"] for a, b in zip(res_h[:-1], res_x))
    print(f"half vs flat top-1 (track, offset) on 40 clean crops of the untrained model: {agree} / 40 agree")
    # windows and their timeline
    rec = torch.cat([tracks[t, :84 * SEG_HOP] for t in (5, 2, 7)])
    win_h, win_u = half.identify_windows(rec, window_s=3.0, hop_s=1.0), f_u.identify_windows(rec, window_s=3.0, hop_s=1.0)
    assert win_h == win_u and len(win_h) > 10
    assert half.timeline(win_h) == f_u.timeline(win_u) and half.timeline(win_h, min_score=0.5) == f_u.timeline(win_u, 0.5)
    # whole recordings
    medley = [torch.cat([tracks[2, :5 * 16000], tracks[5, 2 * 16000:7 * 16000]]), tracks[6], tracks[1, :3000]]
    m_h, m_u = half.match(medley), f_u.match(medley)
    assert m_h == m_u and m_h[0] and m_h[1] and m_h[2] == []
    assert half.match(medley, min_votes=1, min_overlap_s=0.5, top=3) == f_u.match(medley, min_votes=1, min_overlap_s=0.5,
                                                                                  top=3)
    # a live stream in 1 s chunks
    out = {}
    for name, lib in (("half", half), ("f_u", f_u)):
        mon = StreamMonitor(lib, 1, max_chunk_s=1.0)
        wins = []
        for s in range(0, rec.numel(), 16000):
            wins += mon.push([rec[s:s + 16000]])[0]
        wins += mon.end([0])[0]
        out[name] = (wins, mon.timeline(0))
    assert out["half"] == out["f_u"] and len(out["half"][0]) > 10 and out["half"][1]


def test_scores_stay_within_the_rounding_bound_of_the_flat_library(small_libs, dev):
    """Every match that the half library and the flat library over the unrounded rows X both list at the same (track,
    offset) differs in score by at most 2^-9 max||q|| max||x||, the norms taken from the data.  (The worst case of the
    rounding is HALF_SCORE_BOUND = 2^-8 -- bf16 keeps 8 significant bits; the figure asserted here is the tighter one
    the half form was specified with, and real rows stay far inside it because the component errors do not line up.)"""
    cfg, model, tracks, flat, half, f_u = small_libs
    crops = _queries(tracks)[:-1]
    qn = max(float(torch.linalg.norm(flat._embed(flat.segments(c)), dim=1).max()) for c in crops)
    xn = float(torch.linalg.norm(flat.rows(), dim=1).max())
    bound = 2.0 ** -9 * qn * xn
    assert bound <= HALF_SCORE_BOUND * qn * xn
    worst, pairs = 0.0, 0
    for r_h, r_x in zip(half.identify(crops), flat.identify(crops)):
        by_place = {(m["track"], m["offset"]): m["score"] for m in r_x}
        for m in r_h:
            if (m["track"], m["offset"]) in by_place:
                worst = max(worst, abs(m["score"] - by_place[m["track"], m["offset"]]))
                pairs += 1
    print(f"half vs flat: {pairs} common matches, largest score difference {worst:.3e}, bound {bound:.3e} "
          f"(max||q|| {qn:.4f}, max||x|| {xn:.4f})")
    assert pairs >= 1 and worst <= bound, (pairs, worst, bound)


def test_build_add_and_files_of_a_half_library(small_libs, dev, tmp_path):
    cfg, model, tracks, flat, half, f_u = small_libs
    names = [f"song{i}" for i in range(8)]
    built = FingerprintLibrary.build(model, list(tracks), cfg, names=names, max_segments=200, index="half")
    assert built.is_half and built.first.tolist() == flat.first.tolist() and built.names == names
    assert torch.equal(built.half_rows(), ops.rows_to_bf16(flat.rows()))
    grown = FingerprintLibrary.build(model, list(tracks[:5]), cfg, names=names[:5], max_segments=200, index="half")
    flat5 = FingerprintLibrary.build(model, list(tracks[:5]), cfg, names=names[:5], max_segments=200)
    flat5.add(list(tracks[5:]), names=names[5:], max_segments=200)
    assert grown.add(list(tracks[5:]), names=names[5:], max_segments=200) is grown
    assert grown.first.tolist() == flat5.first.tolist() and grown.names == names
    assert torch.equal(grown.half_rows(), ops.rows_to_bf16(flat5.rows())) and grown.nbytes == 260 * grown.n_rows
    # files: the exact list, and the library that comes back answers the same
    crops = _queries(tracks)[:12]
    want = half.identify(crops)
    half.save(str(tmp_path / "lib"))
    assert sorted(os.listdir(tmp_path / "lib")) == ["library.json", "library_half.npy", "library_tracks.npy"]
    assert json.load(open(tmp_path / "lib" / "library.json"))["format"] == 5
    assert np.array_equal(np.load(tmp_path / "lib" / "library_half.npy"), bf16_bits(flat.rows().cpu().numpy()))
    back = FingerprintLibrary.load(str(tmp_path / "lib"), model)
    assert back.is_half and torch.equal(back.half_rows(), half.half_rows()) and back.names == half.names
    assert back.identify(crops) == want and back.nbytes == 260 * back.n_rows
    with pytest.raises(NotImplementedError, match="half"):
        back.rows()
    with pytest.raises(NotImplementedError, match="half"):
        back.self_matches()


# ---- accuracy ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(dev):
    """The briefly trained model of _retrieval_case.build_case, its 24 database tracks (seed 1000 + 0) as a flat library,
    that library halved, and the flat library over the halved rows."""
    case = build_case(dev)
    cfg, model, tracks = case["cfg"], case["model"], synth_tracks(24, 20, 1000, dev)
    flat = FingerprintLibrary.build(model, list(tracks), cfg)
    half = flat.halve()
    f_u = FingerprintLibrary(model, flat.settings, half.half_rows().float(), flat.first, list(flat.names))
    return cfg, model, tracks, flat, half, f_u


@pytest.mark.statistical
def test_top1_accuracy_at_10db_half_against_flat(trained, dev):
    """The queries of test_gpu_identify_pq.py::test_top1_accuracy_at_10db_compact_against_flat (same seeds, 150 per
    length, 1 s and 3 s, white noise at 10 dB) through the flat library and the half one in the same run: the half
    library may lose the dense test's own margins against the flat result of this run, 0.04 at 1 s and 0.03 at 3 s.
    Measured on MI355X: see DESIGN.md 12.32."""
    cfg, model, tracks, flat, half, f_u = trained
    rng = np.random.RandomState(21)
    acc = {}
    for seconds in (1, 3):
        L = seconds * 16000 + 512
        crops, truth = [], []
        for i in range(150):
            t = int(rng.randint(0, 24))
            s0 = int(rng.randint(0, tracks.shape[1] - L))
            crops.append(tracks[t, s0:s0 + L])
            truth.append(t)
        noisy = add_noise(torch.stack(crops), 10.0, 31 + seconds)
        for name, lib in (("flat", flat), ("half", half)):
            res = lib.identify(list(noisy))
            acc[name, seconds] = float(np.mean([bool(r) and r[0]["track"] == t for r, t in zip(res, truth)]))
    print(f"identify top-1 track accuracy at 10 dB: 1 s flat {acc['flat', 1]:.3f} half {acc['half', 1]:.3f}, "
          f"3 s flat {acc['flat', 3]:.3f} half {acc['half', 3]:.3f}")
    assert acc["half", 1] >= acc["flat", 1] - 0.04 and acc["half", 3] >= acc["flat", 3] - 0.03, acc


@pytest.mark.statistical
def test_clean_grid_crops_half_against_flat(trained, dev):
    """The 40 clean grid crops of test_compact_library_agrees_with_the_flat_one_on_clean_crops: how many top-1 (track,
    offset) pairs of the half library agree with the flat library's is printed; asserted is only that each half top-1
    equals that of the flat library over the half library's own rows."""
    cfg, model, tracks, flat, half, f_u = trained
    rng = np.random.RandomState(11)
    crops = []
    for i in range(40):
        L = int(rng.randint(3 * 16000, 5 * 16000))
        j = rng.randint(0, (tracks.shape[1] - L) // SEG_HOP + 1)
        crops.append(tracks[i % 24, j * SEG_HOP:j * SEG_HOP + L])
    res_h, res_u, res_x = half.identify(crops), f_u.identify(crops), flat.identify(crops)
    agree = sum(bool(a) and bool(b) and (a[0]["track"], a[0]["offset"]) == (b[0]["track"], b[0]["offset"])
                for a, b in zip(res_h, res_x))
    shift = max(abs(a[0]["score"] - b[0]["score"]) for a, b in zip(res_h, res_x) if a and b)
    print(f"half vs flat on 40 clean grid crops: {agree} / 40 top-1 (track, offset) pairs agree, "
          f"largest top-1 score difference {shift:.3e}")
    for a, b in zip(res_h, res_u):
        assert a and b and a[0] == b[0], (a[:1], b[:1])
