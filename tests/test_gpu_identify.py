"""Track-aware identification on the MI355X: grafp_identify_f32 against its numpy restatement (tests/_identify_ref.py)
and against ops.seq_rerank, and grafp_amd.library.FingerprintLibrary end to end (build, save / load, from_memmap, windows,
a briefly trained model at 10 dB SNR)."""
import numpy as np
import pytest
import torch

from _identify_ref import identify_ref
from _retrieval_case import add_noise, build_case, synth_tracks
from grafp_amd import fpdb, ops
from grafp_amd.library import FingerprintLibrary
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, rows, first, q, ids, item_row, item_len, top, min_overlap=None, max_len=None):
    out = ops.identify(torch.from_numpy(rows).to(dev), torch.from_numpy(first).to(dev), torch.from_numpy(q).to(dev),
                       torch.from_numpy(ids).to(dev), torch.from_numpy(item_row).to(dev),
                       torch.from_numpy(item_len).to(dev), top=top, min_overlap=min_overlap, max_len=max_len)
    return [t.cpu().numpy() for t in out]


def _dyadic_case(seed, n_items, max_ql, k):
    """Dyadic rows (multiples of 2^-8 in [-1/16, 1/16): every sum is exact) over tracks of random length (zero-row and
    short ones included), track 3 a copy of track 1 and repeated blocks inside track 5 (equal scores), and queries
    planted at random alignments -- straddling track boundaries too -- with random, duplicate and -1 ids around them."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, 60, size=24)
    lens[[0, 7]] = 0
    lens[2] = 3
    lens[1] = lens[3] = 40
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(first[-1])
    rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
    rows[first[3]:first[4]] = rows[first[1]:first[2]]
    if lens[5] >= 8:
        half = lens[5] // 2
        rows[first[5] + half:first[5] + 2 * half] = rows[first[5]:first[5] + half]
    item_len = rng.randint(1, max_ql + 1, size=n_items).astype(np.int32)
    item_len[0] = 0
    item_row = np.concatenate([[0], np.cumsum(item_len[:-1])]).astype(np.int64)
    nq = int(item_len.sum())
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = rng.randint(-1, n, size=(nq, k)).astype(np.int64)
    for i in range(n_items):
        ql, r0 = int(item_len[i]), int(item_row[i])
        a = rng.randint(-ql // 2, n - ql // 2 + 1)
        for s in range(ql):
            if 0 <= a + s < n:
                if rng.rand() < 0.8:
                    q[r0 + s] = rows[a + s]
                ids[r0 + s, 0] = a + s
                if rng.rand() < 0.2:
                    ids[r0 + s, 1] = a + s                       # a duplicate hit
    return rows, first, q, ids, item_row, item_len


@pytest.mark.parametrize("min_overlap", [None, 1, 3])
def test_kernel_matches_restatement_bit_exactly_on_dyadic_inputs(dev, min_overlap):
    rows, first, q, ids, item_row, item_len = _dyadic_case(1 + (min_overlap or 0), 96, 40, 6)
    got = _run(dev, rows, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap)
    want = identify_ref(rows, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap)
    for g, w, name in zip(got, want, ("track", "offset", "score", "votes")):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])
    assert (got[0][:, 0] >= 0).sum() > 40                    # most items found something
    # the same launch with max_len given (asynchronous path)
    again = _run(dev, rows, first, q, ids, item_row, item_len, top=8, min_overlap=min_overlap,
                 max_len=int(item_len.max()))
    assert all(np.array_equal(a, b) for a, b in zip(again, got))


def test_kernel_matches_restatement_at_the_size_limits(dev):
    """ql = 256 with k = 32 (8192 keys: the query rows no longer fit the LDS next to the slots and are read from global
    memory) and a small item in the same launch."""
    rows, first, q, ids, item_row, item_len = _dyadic_case(7, 3, 256, 32)
    item_len[:] = [256, 5, 200]
    item_row = np.array([0, 256, 261], np.int64)
    nq = 461
    rng = np.random.RandomState(8)
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = rng.randint(-1, rows.shape[0], size=(nq, 32)).astype(np.int64)
    ids[:, 5] = np.arange(nq) % rows.shape[0]                # long runs of one alignment
    for mo in (None, 1):
        got = _run(dev, rows, first, q, ids, item_row, item_len, top=16, min_overlap=mo)
        want = identify_ref(rows, first, q, ids, item_row, item_len, top=16, min_overlap=mo)
        for g, w, name in zip(got, want, ("track", "offset", "score", "votes")):
            assert np.array_equal(g, w), (mo, name, np.argwhere(g != w)[:5])


def test_kernel_matches_restatement_on_unit_rows_over_200_tracks(dev):
    rng = np.random.RandomState(3)
    lens = rng.randint(0, 80, size=200)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(first[-1])
    rows = rng.randn(n, 128).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    n_items, k = 300, 10
    item_len = rng.randint(1, 32, size=n_items).astype(np.int32)
    item_row = np.concatenate([[0], np.cumsum(item_len[:-1])]).astype(np.int64)
    q = np.empty((int(item_len.sum()), 128), np.float32)
    for i in range(n_items):
        ql, r0 = int(item_len[i]), int(item_row[i])
        if i % 3 == 2:                                         # a decoy that straddles a track boundary
            t = rng.randint(1, 200)
            a = int(first[t]) - ql // 2
        else:
            t = rng.randint(0, 200)
            a = int(first[t]) + rng.randint(0, max(1, lens[t] - ql + 1))
        src = rows[np.clip(np.arange(a, a + ql), 0, n - 1)]
        noisy = src + 0.3 * rng.randn(ql, 128).astype(np.float32)
        q[r0:r0 + ql] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
    index = ops.FlatL2Index(device=dev)
    index.add(torch.from_numpy(rows).to(dev))
    _, ids_t = index.search(torch.from_numpy(q).to(dev), k)
    ids = ids_t.cpu().numpy()
    for mo in (None, 4):
        tr, off, sc, vo = _run(dev, rows, first, q, ids, item_row, item_len, top=5, min_overlap=mo)
        wt, wo, ws, wv = identify_ref(rows, first, q, ids, item_row, item_len, top=5, min_overlap=mo)
        for i in range(n_items):
            got = {int(t): (int(o), float(s), int(v)) for t, o, s, v in zip(tr[i], off[i], sc[i], vo[i]) if t >= 0}
            want = {int(t): (int(o), float(s), int(v)) for t, o, s, v in zip(wt[i], wo[i], ws[i], wv[i]) if t >= 0}
            assert len(got) == len(want), i
            cut = min((s for _, s, _ in want.values()), default=0.0)
            for t in set(got) | set(want):
                if t in got and t in want:
                    assert got[t][0] == want[t][0] and got[t][2] == want[t][2], (i, t, got[t], want[t])
                    assert abs(got[t][1] - want[t][1]) <= 1e-6, (i, t, got[t], want[t])
                else:                                          # at the cut-off of the top list: a near tie
                    s = (got.get(t) or want.get(t))[1]
                    assert abs(s - cut) <= 4e-6, (i, t, s, cut)
            assert np.all(np.diff(sc[i][tr[i] >= 0]) <= 0)
            for j in range(int((tr[i] >= 0).sum())):
                if tr[i, j] != wt[i, j]:
                    assert abs(float(ws[i, j]) - float(sc[i, j])) <= 4e-6 + 1e-6, (i, j)
        assert (tr[:, 0] >= 0).mean() > 0.6


def test_top1_matches_seq_rerank_on_a_one_track_library(dev):
    rng = np.random.RandomState(5)
    n, n_items, k = 500, 200, 10
    rows = rng.randn(n, 128).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    item_len = rng.randint(1, 41, size=n_items).astype(np.int32)
    item_row = np.concatenate([[0], np.cumsum(item_len[:-1])]).astype(np.int64)
    nq = int(item_len.sum())
    q = rng.randn(nq, 128).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    ids = np.empty((nq, k), np.int64)
    for i in range(n_items):
        ql, r0 = int(item_len[i]), int(item_row[i])
        a = rng.randint(0, n - ql + 1, size=(ql, k))          # every alignment in [0, n - ql]
        a[:, 0] = a[0, 0]
        ids[r0:r0 + ql] = a + np.arange(ql)[:, None]
    t = lambda a: torch.from_numpy(a).to(dev)
    tr, off, sc, _ = ops.identify(t(rows), t(np.array([0, n], np.int64)), t(q), t(ids), t(item_row), t(item_len), top=1)
    ri, rs = ops.seq_rerank(t(rows), t(q), t(ids), t(item_row), t(item_len), top=1)
    assert (tr.cpu().numpy() == 0).all()
    assert np.array_equal(off.cpu().numpy()[:, 0].astype(np.int64), ri.cpu().numpy()[:, 0])
    assert np.array_equal(sc.cpu().numpy()[:, 0].view(np.uint32), rs.cpu().numpy()[:, 0].view(np.uint32))


# ---- the library end to end ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_lib(dev):
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    tracks = synth_tracks(8, 84 * SEG_HOP / 16000, 4242, dev)            # 8.06 s: a whole number of segment hops
    lib = FingerprintLibrary.build(model, list(tracks), cfg, names=[f"song{i}" for i in range(8)], max_segments=200)
    return cfg, model, tracks, lib


def test_build_track_table_counts_unfold_segments(small_lib, dev):
    cfg, model, tracks, lib = small_lib
    step = int(cfg["n_frames"] * (1 - cfg["overlap"]))
    want = [ops.unfold_segments(ops.logmel(x, cfg["fs"], cfg["n_fft"], cfg["win_len"], cfg["hop_len"], cfg["n_mels"]),
                                cfg["n_frames"], step).shape[0] for x in tracks]
    assert np.diff(lib.first).tolist() == want and lib.n_rows == sum(want)
    # short tracks: zero rows, kept in the table, never matched
    lib2 = FingerprintLibrary.build(model, [tracks[0], tracks[1][:4000], tracks[2]], cfg, precision="f32")
    assert np.diff(lib2.first)[1] == 0 and lib2.n_tracks == 3
    res = lib2.identify(tracks[1][:4000])
    assert res == []


def test_clean_grid_crops_are_identified(small_lib, dev):
    cfg, model, tracks, lib = small_lib
    rng = np.random.RandomState(11)
    crops, truth = [], []
    for i in range(40):
        t = i % 8
        L = int(rng.randint(3 * 16000, 5 * 16000))
        j = rng.randint(0, (tracks.shape[1] - L) // SEG_HOP + 1)
        crops.append(tracks[t, j * SEG_HOP:j * SEG_HOP + L])
        truth.append((t, j))
    crops.append(tracks[0, :3000])                                      # shorter than one segment
    res = lib.identify(crops)
    assert res[-1] == []
    for (t, j), r in zip(truth, res[:-1]):
        assert r and r[0]["track"] == t and r[0]["name"] == f"song{t}", (t, j, r[:2])
        assert abs(r[0]["offset"] - j) <= 1, (t, j, r[0])
        assert r[0]["offset_s"] == r[0]["offset"] * SEG_HOP / 16000
    # one waveform in -> one list out; a different input rate is resampled
    one = lib.identify(crops[0])
    assert one[0]["track"] == truth[0][0]
    up = ops.resample(crops[3].contiguous(), [0], [crops[3].numel()], 16000, 22050)[0]
    assert lib.identify([up], fs=22050)[0][0]["track"] == truth[3][0]


def test_save_load_and_from_memmap_round_trip(small_lib, dev, tmp_path):
    cfg, model, tracks, lib = small_lib
    queries = [tracks[i % 8, 2000 * i:2000 * i + 50000] for i in range(16)]
    want = lib.identify(queries)
    lib.save(str(tmp_path / "lib"))
    back = FingerprintLibrary.load(str(tmp_path / "lib"), model)
    assert torch.equal(back.rows(), lib.rows()) and back.names == lib.names
    assert back.identify(queries) == want
    # create_dummy_db (eval mode, no augmentation, the same packing) + a track table == build in f32
    from grafp_amd.modules.transformations import GPUTransformNeuralfp
    built = FingerprintLibrary.build(model, list(tracks), cfg, precision="f32", max_segments=200)
    fpdb.create_dummy_db([x[None] for x in tracks], GPUTransformNeuralfp(cfg, None, None, train=False), model,
                         str(tmp_path), fname="dummy_db", verbose=False, max_segments=200)
    mm = FingerprintLibrary.from_memmap(str(tmp_path), "dummy_db", np.diff(built.first), model, cfg)
    assert torch.equal(mm.rows(), built.rows())
    assert mm.identify(queries) == built.identify(queries)


@pytest.fixture(scope="module")
def trained(dev):
    """The briefly trained model of _retrieval_case.build_case and its 24 database tracks (seed 1000 + 0)."""
    case = build_case(dev)
    return case["cfg"], case["model"], synth_tracks(24, 20, 1000, dev)


def test_windows_and_timeline(trained, dev):
    """Three library tracks back to back, a 3 s window every second.  (A trained model: an untrained net maps every
    segment to nearly the same fingerprint, so the windows that straddle a boundary score as high as true matches.)"""
    cfg, model, tracks = trained
    tracks = tracks[:8, :84 * SEG_HOP]                               # 8.06 s each: a whole number of segment hops
    lib = FingerprintLibrary.build(model, list(tracks), cfg, max_segments=200)
    order = [5, 2, 7]
    rec = torch.cat([tracks[t] for t in order])
    dur = tracks.shape[1] / 16000
    windows = lib.identify_windows(rec, window_s=3.0, hop_s=1.0)
    assert len(windows) == int((3 * dur - 3.0) // 1.0) + 1
    assert [w["start_s"] for w in windows[:3]] == [0.0, 1.0, 2.0] and windows[0]["end_s"] == 3.0
    spans = lib.timeline(windows, min_score=0.9)
    assert [s["track"] for s in spans] == order, spans
    for k, s in enumerate(spans):
        assert abs(s["start_s"] - k * dur) <= 1.0 + 1e-9 and abs(s["end_s"] - (k + 1) * dur) <= 1.0 + 1e-9, spans
        assert abs(s["track_offset_s"] - (s["start_s"] - k * dur)) <= lib.segment_s + 1e-6, s
        assert s["name"] == f"track{order[k]}" and s["score"] > 0.9


@pytest.mark.statistical
def test_top1_accuracy_of_a_trained_model_at_10db(trained, dev):
    """The briefly trained model of _retrieval_case, its 24 database tracks as the library (bf16), 150 queries per
    length cut at random sample offsets (off the segment grid) with white noise at 10 dB SNR.  Measured on MI355X:
    1 s 0.960, 3 s 1.000 (training is bit-reproducible, so every lease measures the same)."""
    cfg, model, tracks = trained
    lib = FingerprintLibrary.build(model, list(tracks), cfg)
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
        res = lib.identify(list(noisy))
        acc[seconds] = float(np.mean([bool(r) and r[0]["track"] == t for r, t in zip(res, truth)]))
    print(f"identify top-1 track accuracy at 10 dB: 1 s {acc[1]:.3f}, 3 s {acc[3]:.3f}")
    assert acc[1] >= ACC_BAR[1] and acc[3] >= ACC_BAR[3], acc


ACC_BAR = {1: 0.90, 3: 0.97}          # measured 0.960 / 1.000, minus a margin of 4 and 3 queries in 100
