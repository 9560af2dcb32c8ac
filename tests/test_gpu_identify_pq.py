"""Identification against IVF-PQ codes on the MI355X: grafp_identify_pq_f32 against its restatement (tests/_identify_ref.py
on the rows tests/_identify_pq_ref.py decodes) and against ops.identify on the decoded rows, ivfpq.IVFPQIndex without raw
rows, and the compact form of grafp_amd.library.FingerprintLibrary end to end."""
import numpy as np
import pytest
import torch

from _identify_pq_ref import decode
from _identify_ref import identify_ref
from _retrieval_case import add_noise, build_case, synth_tracks
from grafp_amd import ops
from grafp_amd.ivfpq import IVFPQIndex
from grafp_amd.library import FingerprintLibrary

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
NAMES = ("track", "offset", "score", "votes")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, a, codes, cent, books, first, q, ids, item_row, item_len, top, min_overlap=None, max_len=None):
    t = lambda x: torch.from_numpy(x).to(dev)
    out = ops.identify_pq(t(a), t(codes), t(cent), t(books), t(first), t(q), t(ids), t(item_row), t(item_len), top=top,
                          min_overlap=min_overlap, max_len=max_len)
    return [x.cpu().numpy() for x in out]


def _dyadic_case(seed, n_items, max_ql, k, M, nlist=7):
    """tests/test_gpu_identify.py's _dyadic_case on codes.  Centroids and codewords are multiples of 2^-8 in
    [-1/32, 1/32), so decoded rows are multiples of 2^-8 in [-1/16, 1/16) like the queries, and every product and sum of
    a score is exact in f32 (at most 256 * 128 products of at most 2^-8, in steps of 2^-16: 23 bits).  Random codes over
    tracks of random length (zero-row and short ones included), track 3 a copy of track 1's codes and list ids and a
    repeated block inside track 5 (equal scores), queries planted at random alignments -- straddling track boundaries
    too -- with random, duplicate and -1 ids around them."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, 60, size=24)
    lens[[0, 7]] = 0
    lens[2] = 3
    lens[1] = lens[3] = 40
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(first[-1])
    cent = (rng.randint(-8, 8, size=(nlist, 128)) / 256.0).astype(np.float32)
    books = (rng.randint(-8, 8, size=(M, 256, 128 // M)) / 256.0).astype(np.float32)
    a = rng.randint(0, nlist, size=n).astype(np.int32)
    codes = rng.randint(0, 256, size=(n, M)).astype(np.uint8)
    a[first[3]:first[4]], codes[first[3]:first[4]] = a[first[1]:first[2]], codes[first[1]:first[2]]
    if lens[5] >= 8:
        half = lens[5] // 2
        a[first[5] + half:first[5] + 2 * half] = a[first[5]:first[5] + half]
        codes[first[5] + half:first[5] + 2 * half] = codes[first[5]:first[5] + half]
    rows = decode(a, codes, cent, books)
    item_len = rng.randint(1, max_ql + 1, size=n_items).astype(np.int32)
    item_len[0] = 0
    item_row = np.concatenate([[0], np.cumsum(item_len[:-1])]).astype(np.int64)
    nq = int(item_len.sum())
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = rng.randint(-1, n, size=(nq, k)).astype(np.int64)
    for i in range(n_items):
        ql, r0 = int(item_len[i]), int(item_row[i])
        al = rng.randint(-ql // 2, n - ql // 2 + 1)
        for s in range(ql):
            if 0 <= al + s < n:
                if rng.rand() < 0.8:
                    q[r0 + s] = rows[al + s]
                ids[r0 + s, 0] = al + s
                if rng.rand() < 0.2:
                    ids[r0 + s, 1] = al + s                      # a duplicate hit
    return (a, codes, cent, books), rows, first, q, ids, item_row, item_len


@pytest.mark.parametrize("M", [16, 32, 64, 128])
@pytest.mark.parametrize("min_overlap", [None, 1, 3])
def test_kernel_matches_restatement_bit_exactly_on_dyadic_inputs(dev, min_overlap, M):
    pq, rows, first, q, ids, item_row, item_len = _dyadic_case(1 + (min_overlap or 0) + M, 96, 40, 6, M)
    got = _run(dev, *pq, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap)
    want = identify_ref(rows, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap)
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, np.argwhere(g != w)[:5])
    assert (got[0][:, 0] >= 0).sum() > 40                    # most items found something
    assert (got[0][0] == -1).all() and (got[1][0] == np.iinfo(np.int32).min).all()       # the empty item: padding
    assert np.isneginf(got[2][0]).all() and (got[3][0] == 0).all()
    # the same launch with max_len given (asynchronous path)
    again = _run(dev, *pq, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap,
                 max_len=int(item_len.max()))
    assert all(np.array_equal(x, y) for x, y in zip(again, got))
    # and ops.identify on the decoded rows: the same bits
    t = lambda x: torch.from_numpy(x).to(dev)
    flat = ops.identify(t(rows), t(first), t(q), t(ids), t(item_row), t(item_len), top=8, min_overlap=min_overlap)
    for g, f, name in zip(got, flat, NAMES):
        assert np.array_equal(g.view(np.uint32), f.cpu().numpy().view(np.uint32)), name


@pytest.mark.parametrize("M", [16, 32, 64, 128])
def test_kernel_matches_restatement_at_the_size_limits(dev, M):
    """ql = 256 with k = 32 (8192 keys: the query rows no longer fit the LDS next to the slots and are read from global
    memory), a small item and a 200-segment one in the same launch."""
    pq, rows, first, _, _, _, _ = _dyadic_case(7 + M, 3, 256, 32, M)
    item_len = np.array([256, 5, 200], np.int32)
    item_row = np.array([0, 256, 261], np.int64)
    nq = 461
    rng = np.random.RandomState(8)
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = rng.randint(-1, rows.shape[0], size=(nq, 32)).astype(np.int64)
    ids[:, 5] = np.arange(nq) % rows.shape[0]                # long runs of one alignment
    for mo in (None, 1):
        got = _run(dev, *pq, first, q, ids, item_row, item_len, top=16, min_overlap=mo)
        want = identify_ref(rows, first, q, ids, item_row, item_len, top=16, min_overlap=mo)
        for g, w, name in zip(got, want, NAMES):
            assert np.array_equal(g, w), (mo, name, np.argwhere(g != w)[:5])


@pytest.fixture(scope="module")
def unit_case():
    """About 2 200 random unit rows over 60 tracks of 0-79 rows; 120 items of 1-31 rows cut inside tracks, plus
    0.3 * N(0, I) noise, renormalised.  -> rows, first, q, item_row, item_len, truth (track, offset) per item."""
    rng = np.random.RandomState(3)
    lens = rng.randint(0, 80, size=60)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(first[-1])
    rows = rng.randn(n, 128).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    n_items = 120
    item_len = rng.randint(1, 32, size=n_items).astype(np.int32)
    item_row = np.concatenate([[0], np.cumsum(item_len[:-1])]).astype(np.int64)
    q = np.empty((int(item_len.sum()), 128), np.float32)
    truth = []
    for i in range(n_items):
        ql, r0 = int(item_len[i]), int(item_row[i])
        t = int(rng.choice(np.nonzero(lens >= ql)[0]))           # cut inside a track
        off = int(rng.randint(0, lens[t] - ql + 1))
        src = rows[first[t] + off:first[t] + off + ql]
        noisy = src + 0.3 * rng.randn(ql, 128).astype(np.float32)
        q[r0:r0 + ql] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
        truth.append((t, off))
    return rows, first, q, item_row, item_len, np.array(truth)


def test_trained_quantiser_on_unit_rows(dev, unit_case):
    """About 2 200 unit rows over 60 tracks in a trained IVFPQIndex(nlist=8, M=64, keep_raw=False): identify_pq is
    ops.identify on index.reconstruct() bit for bit, the restatement within the tolerances of
    test_gpu_identify.py::test_kernel_matches_restatement_on_unit_rows_over_200_tracks, and names the true track and
    offset for most items."""
    rows, first, q, item_row, item_len, truth = unit_case
    n_items, k = len(item_row), 10
    index = IVFPQIndex(nlist=8, M=64, device=dev, keep_raw=False)
    index.train(torch.from_numpy(rows).to(dev))
    index.add(torch.from_numpy(rows).to(dev))
    with pytest.raises(RuntimeError, match="keep_raw=False"):
        index.rows()
    a_t, codes_t = index.codes_by_row()
    assert a_t.dtype == torch.int32 and codes_t.dtype == torch.uint8 and tuple(codes_t.shape) == (rows.shape[0], 64)
    quant = index.quantiser()
    cent, books = quant["centroids"], quant["codebooks"]
    dec_t = index.reconstruct()
    dec = decode(a_t.cpu().numpy(), codes_t.cpu().numpy(), cent.cpu().numpy(), books.cpu().numpy())
    assert np.array_equal(dec_t.cpu().numpy(), dec)
    assert torch.equal(index.reconstruct(ids=[5, 0, 77]), dec_t[[5, 0, 77]])
    t = lambda x: torch.from_numpy(x).to(dev)
    for nprobe in (8, 3):
        index.nprobe = nprobe
        _, ids_t = index.search(t(q), k)
        ids = ids_t.cpu().numpy()
        for mo in (None, 4):
            got_t = ops.identify_pq(a_t, codes_t, cent, books, t(first), t(q), ids_t, t(item_row), t(item_len), top=5,
                                    min_overlap=mo)
            flat_t = ops.identify(dec_t, t(first), t(q), ids_t, t(item_row), t(item_len), top=5, min_overlap=mo)
            tr, off, sc, vo = (x.cpu().numpy() for x in got_t)
            for g, f, name in zip((tr, off, sc, vo), flat_t, NAMES):
                f = f.cpu().numpy()
                assert np.array_equal(g.view(np.uint32), f.view(np.uint32)), (nprobe, mo, name)
            wt, wo, ws, wv = identify_ref(dec, first, q, ids, item_row, item_len, top=5, min_overlap=mo)
            for i in range(n_items):
                got = {int(t_): (int(o), float(s), int(v)) for t_, o, s, v in zip(tr[i], off[i], sc[i], vo[i]) if t_ >= 0}
                want = {int(t_): (int(o), float(s), int(v)) for t_, o, s, v in zip(wt[i], wo[i], ws[i], wv[i]) if t_ >= 0}
                assert len(got) == len(want), i
                cut = min((s for _, s, _ in want.values()), default=0.0)
                for t_ in set(got) | set(want):
                    if t_ in got and t_ in want:
                        assert got[t_][0] == want[t_][0] and got[t_][2] == want[t_][2], (i, t_, got[t_], want[t_])
                        assert abs(got[t_][1] - want[t_][1]) <= 1e-6, (i, t_, got[t_], want[t_])
                    else:                                          # at the cut-off of the top list: a near tie
                        s = (got.get(t_) or want.get(t_))[1]
                        assert abs(s - cut) <= 4e-6, (i, t_, s, cut)
                assert np.all(np.diff(sc[i][tr[i] >= 0]) <= 0)
                for j in range(int((tr[i] >= 0).sum())):
                    if tr[i, j] != wt[i, j]:
                        assert abs(float(ws[i, j]) - float(sc[i, j])) <= 4e-6 + 1e-6, (i, j)
            right = float(np.mean((tr[:, 0] == truth[:, 0]) & (off[:, 0] == truth[:, 1])))
            print(f"identify_pq on unit rows: nprobe {nprobe} min_overlap {mo}: top-1 track and offset right {right:.3f}")
            assert right > 0.6, (nprobe, mo, right)


def test_index_without_raw_rows_searches_like_the_one_with(dev, unit_case):
    rows, _, q, _, _, _ = unit_case
    out = []
    for keep in (True, False):
        index = IVFPQIndex(nlist=8, M=64, device=dev, keep_raw=keep)
        index.train(torch.from_numpy(rows).to(dev))
        index.add(torch.from_numpy(rows[:1000]).to(dev))
        index.add(torch.from_numpy(rows[1000:]).to(dev))
        index.nprobe = 3
        out.append((index, *index.search(torch.from_numpy(q).to(dev), 10)))
    (raw, D0, I0), (bare, D1, I1) = out
    assert torch.equal(D0, D1) and torch.equal(I0, I1) and (I0 >= 0).any()
    assert torch.equal(raw.rows(), torch.from_numpy(rows).to(dev)) and bare._raw == []
    assert all(torch.equal(x, y) for x, y in zip(raw.codes_by_row(), bare.codes_by_row()))
    # from_codes: the same index again, nothing re-encoded
    again = IVFPQIndex.from_codes(bare.quantiser(), *bare.codes_by_row(), device=dev, nprobe=3)
    assert not again.keep_raw and again.ntotal == rows.shape[0]
    D2, I2 = again.search(torch.from_numpy(q).to(dev), 10)
    assert torch.equal(D2, D1) and torch.equal(I2, I1)


# ---- the library end to end ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(dev):
    """The briefly trained model of _retrieval_case.build_case, its 24 database tracks (seed 1000 + 0) as a flat library
    and that library compressed."""
    case = build_case(dev)
    cfg, model, tracks = case["cfg"], case["model"], synth_tracks(24, 20, 1000, dev)
    flat = FingerprintLibrary.build(model, list(tracks), cfg)
    compact = flat.compress(nlist=16, nprobe=8)
    return cfg, model, tracks, flat, compact


def test_compact_library_agrees_with_the_flat_one_on_clean_crops(trained, dev, tmp_path):
    cfg, model, tracks, flat, compact = trained
    assert compact.is_compact and not flat.is_compact and compact.n_rows == flat.n_rows
    assert compact.first.tolist() == flat.first.tolist() and compact.names == flat.names
    rng = np.random.RandomState(11)
    crops, truth = [], []
    for i in range(40):
        t = i % 24
        L = int(rng.randint(3 * 16000, 5 * 16000))
        j = rng.randint(0, (tracks.shape[1] - L) // SEG_HOP + 1)
        crops.append(tracks[t, j * SEG_HOP:j * SEG_HOP + L])
        truth.append((t, j))
    res_f, res_c = flat.identify(crops), compact.identify(crops)
    for (t, j), r in zip(truth, res_f):                       # first the flat library itself
        assert r and r[0]["track"] == t and abs(r[0]["offset"] - j) <= 1, (t, j, r[:2])
    for rf, rc in zip(res_f, res_c):
        assert rc and rc[0]["track"] == rf[0]["track"] and rc[0]["offset"] == rf[0]["offset"], (rf[:2], rc[:2])
        assert rc[0]["name"] == rf[0]["name"] and rc[0]["offset_s"] == rf[0]["offset_s"]
    shift = np.array([abs(rc[0]["score"] - rf[0]["score"]) for rf, rc in zip(res_f, res_c)])
    low = min(rc[0]["score"] for rc in res_c)
    print(f"compact vs flat top-1 score on 40 clean crops: max shift {shift.max():.4f}, mean {shift.mean():.4f}; "
          f"lowest compact top-1 score {low:.4f}, lowest flat {min(rf[0]['score'] for rf in res_f):.4f}")
    # files: save / load gives the same answers
    compact.save(str(tmp_path / "lib"))
    back = FingerprintLibrary.load(str(tmp_path / "lib"), model)
    assert back.is_compact and all(torch.equal(x, y) for x, y in zip(back.codes(), compact.codes()))
    assert back.identify(crops) == res_c
    with pytest.raises(NotImplementedError, match="flat form"):
        compact.self_matches()
    with pytest.raises(NotImplementedError, match="flat form"):
        compact.rows()


def test_build_with_a_given_quantiser_encodes_like_compress_and_the_bytes_per_row(trained, dev):
    cfg, model, tracks, flat, compact = trained
    built = FingerprintLibrary.build(model, list(tracks), cfg, index="ivfpq", quantiser=compact.quantiser(), nprobe=8)
    assert built.is_compact and built.first.tolist() == compact.first.tolist()
    assert all(torch.equal(x, y) for x, y in zip(built.codes(), compact.codes()))
    # streaming build that trains on its own first rows: same table, a usable library
    own = FingerprintLibrary.build(model, list(tracks), cfg, index="ivfpq", nlist=16, nprobe=8, train_rows=1500,
                                   max_segments=400)
    assert own.first.tolist() == flat.first.tolist() and own.codes()[1].shape == compact.codes()[1].shape
    r = own.identify(tracks[3, 10 * SEG_HOP:10 * SEG_HOP + 4 * 16000])
    assert r and r[0]["track"] == 3 and abs(r[0]["offset"] - 10) <= 1
    # add() on a compact library encodes with its quantiser
    more = FingerprintLibrary.build(model, list(tracks[:20]), cfg, index="ivfpq", quantiser=compact.quantiser(), nprobe=8)
    more.add(list(tracks[20:]))
    assert more.first.tolist() == compact.first.tolist()
    assert all(torch.equal(x, y) for x, y in zip(more.codes(), compact.codes()))
    # bytes: row-order codes, the list-ordered copy, the ids and the list ids
    M, n = 64, compact.n_rows
    quant = sum(v.numel() * 4 for v in compact.quantiser().values())
    print(f"bytes per row: flat {flat.nbytes / n:.1f}, compact {(compact.nbytes - quant) / n:.1f} + {quant} of quantiser")
    assert compact.nbytes <= n * (2 * M + 24) + quant
    assert flat.nbytes == n * 772


def test_windows_and_timeline_agree_with_the_flat_library(trained, dev):
    cfg, model, tracks, flat, compact = trained
    order = [5, 2, 7]
    rec = torch.cat([tracks[t, :84 * SEG_HOP] for t in order])
    spans_f = flat.timeline(flat.identify_windows(rec, window_s=3.0, hop_s=1.0), min_score=0.9)
    spans_c = compact.timeline(compact.identify_windows(rec, window_s=3.0, hop_s=1.0), min_score=0.9)
    assert [s["track"] for s in spans_f] == order, spans_f
    assert [s["track"] for s in spans_c] == [s["track"] for s in spans_f], spans_c


@pytest.mark.statistical
def test_top1_accuracy_at_10db_compact_against_flat(trained, dev):
    """The queries of test_gpu_identify.py::test_top1_accuracy_of_a_trained_model_at_10db (same seeds, 150 per length,
    1 s and 3 s, white noise at 10 dB) through the flat library and the compact one (nlist 16, M 64, nprobe 8) in the
    same run: the compact library may lose ACC_BAR's own margins against the flat result of this run, 0.04 at 1 s and
    0.03 at 3 s.  Measured on MI355X (training is bit-reproducible): 1 s flat 0.960, compact 0.967; 3 s flat 1.000,
    compact 1.000."""
    cfg, model, tracks, flat, compact = trained
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
        for name, lib in (("flat", flat), ("compact", compact)):
            res = lib.identify(list(noisy))
            acc[name, seconds] = float(np.mean([bool(r) and r[0]["track"] == t for r, t in zip(res, truth)]))
    print(f"identify top-1 track accuracy at 10 dB: 1 s flat {acc['flat', 1]:.3f} compact {acc['compact', 1]:.3f}, "
          f"3 s flat {acc['flat', 3]:.3f} compact {acc['compact', 3]:.3f}")
    assert acc["compact", 1] >= acc["flat", 1] - 0.04 and acc["compact", 3] >= acc["flat", 3] - 0.03, acc
