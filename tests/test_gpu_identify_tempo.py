"""Identification of recordings that play faster or slower than the catalogue, on the MI355X: grafp_identify_tempo_f32
against its numpy restatement (tests/_identify_tempo_ref.py) and against grafp_identify_f32 at the one ratio 256, at the
limits of its launch plans and of the merge, on unit rows planted along a slope, and FingerprintLibrary.identify(tempo=...)
end to end (an untrained model, then a briefly trained one at 10 dB SNR)."""
import numpy as np
import pytest
import torch

from _identify_tempo_ref import tempo_case, tempo_ref, w
from _retrieval_case import add_noise, build_case, synth_tracks
from grafp_amd import ops
from grafp_amd.library import FingerprintLibrary, tempo_ratios
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
NAMES = ("track", "offset", "score", "votes", "ratio")
# the ratio sets of the dyadic test, with the items each gets (the restatement's cost grows with both)
RATIO_SETS = {"one": ([256], 64), "three": ([243, 256, 269], 64), "nine": (list(range(240, 273, 4)), 40),
              "ends": ([128, 256, 512], 64), "sixty-four": (list(range(225, 289)), 10)}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, rows, first, q, ids, item_row, item_len, ratios, top, min_overlap=None, max_len=None):
    t = lambda a: torch.from_numpy(a).to(dev)
    out = ops.identify_tempo(t(rows), t(first), t(q), t(ids), t(item_row), t(item_len), ratios, top=top,
                             min_overlap=min_overlap, max_len=max_len)
    return [o.cpu().numpy() for o in out]


def _dense(dev, rows, first, q, ids, item_row, item_len, top, min_overlap=None):
    t = lambda a: torch.from_numpy(a).to(dev)
    out = ops.identify(t(rows), t(first), t(q), t(ids), t(item_row), t(item_len), top=top, min_overlap=min_overlap)
    return [o.cpu().numpy() for o in out]


def _same(got, want, what=""):
    for g, x, name in zip(got, want, NAMES):
        assert g.dtype == x.dtype and np.array_equal(g, x), (what, name, np.argwhere(g != x)[:5])


@pytest.mark.parametrize("min_overlap", [None, 1, 3])
@pytest.mark.parametrize("which", list(RATIO_SETS))
def test_kernel_matches_restatement_bit_exactly_on_dyadic_inputs(dev, which, min_overlap):
    ratios, n_items = RATIO_SETS[which]
    case = tempo_case(1 + (min_overlap or 0) + 10 * len(ratios), ratios, n_items, 40, 6)
    got = _run(dev, *case, ratios, top=8, min_overlap=min_overlap)
    want = tempo_ref(*case, ratios, top=8, min_overlap=min_overlap)
    found = int((got[0][:, 0] >= 0).sum())
    used = sorted(set(got[4][got[0] >= 0].tolist()))
    print(f"{which} min_overlap={min_overlap}: {found} of {n_items} items find something, winning ratios {used}")
    _same(got, want)
    assert found > n_items // 2
    assert len(used) > 1 or len(ratios) == 1                 # more than one ratio wins somewhere
    # the same launch with max_len given (asynchronous path), as an upper bound too
    item_len = case[5]
    for max_len in (int(item_len.max()), int(item_len.max()) + 9):
        again = _run(dev, *case, ratios, top=8, min_overlap=min_overlap, max_len=max_len)
        assert all(np.array_equal(a, b) for a, b in zip(again, got)), max_len


@pytest.mark.parametrize("min_overlap", [None, 1, 3])
def test_the_ratio_one_is_the_dense_kernel_bit_for_bit(dev, min_overlap):
    case = tempo_case(40 + (min_overlap or 0), [256], 96, 40, 6)
    got = _run(dev, *case, [256], top=8, min_overlap=min_overlap)
    dense = _dense(dev, *case, top=8, min_overlap=min_overlap)
    for g, x, name in zip(got, dense, NAMES):
        assert np.array_equal(g.view(np.int32), x.view(np.int32)), name
    assert np.array_equal(got[4], np.where(got[0] >= 0, 256, 0))
    assert (got[0][:, 0] >= 0).sum() > 40


def _limit_case(lens, k, seed, ratios):
    """Items of the given lengths over tempo_case's 24 tracks: random dyadic query rows and ids, one column of hits that
    walks the library at the first ratio (long runs of one alignment)."""
    rows, first, _, _, _, _ = tempo_case(seed, ratios, 3, 8, 6)
    n = rows.shape[0]
    item_len = np.array(lens, np.int32)
    item_row = np.concatenate([[0], np.cumsum(item_len[:-1])]).astype(np.int64)
    nq = int(item_len.sum())
    rng = np.random.RandomState(seed + 1)
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = rng.randint(-1, n, size=(nq, k)).astype(np.int64)
    for r0, ql in zip(item_row, item_len):
        ids[r0:r0 + ql, k // 2] = (int(r0) + w(np.arange(ql), ratios[0])) % n
    return rows, first, q, ids, item_row, item_len


def test_query_rows_from_global_memory_at_the_largest_item(dev):
    """ql = 256 with k = 32 (8192 keys: the query rows no longer fit the LDS next to the slots) and two smaller items in
    the same launch, two ratios."""
    ratios = [230, 282]
    case = _limit_case([256, 5, 90], 32, 7, ratios)
    got = _run(dev, *case, ratios, top=16, min_overlap=1)          # every candidate with a pair is scored
    _same(got, tempo_ref(*case, ratios, top=16, min_overlap=1))
    assert (got[0][:, 0] >= 0).all()


def test_both_plans_at_the_lds_switch(dev):
    """identify_plan keeps the query rows in LDS while 16 * Pmax + max_len * 512 fits 160 KiB - 256: with 4096 slots that
    is max_len <= 191.  The same items with max_len 191 (LDS, its largest) and 192 (global) give the same bits."""
    ratios = [250, 256, 262]
    case = _limit_case([191, 0, 17], 21, 9, ratios)
    want = tempo_ref(*case, ratios, top=8, min_overlap=2)
    for max_len in (191, 192):
        assert 191 * 21 <= 4096 and 192 * 21 <= 4096
        _same(_run(dev, *case, ratios, top=8, min_overlap=2, max_len=max_len), want, max_len)
    _same(_run(dev, *case, ratios, top=8, min_overlap=2), want)
    assert want[0][1, 0] == -1 and want[4][1, 0] == 0          # the item of length 0 finds nothing


def test_the_merge_at_its_4096_entries_and_the_empty_launch(dev):
    ratios = list(range(225, 289))
    case = tempo_case(77, ratios, 6, 12, 6)
    got = _run(dev, *case, ratios, top=64, min_overlap=1)
    _same(got, tempo_ref(*case, ratios, top=64, min_overlap=1))
    assert got[0].shape == (6, 64) and (got[0][1:, 0] >= 0).all() and (got[0][:, -1] == -1).all()   # 24 tracks only
    assert (got[2][0] == -np.inf).all() and (got[1][0] == np.iinfo(np.int32).min).all()             # item 0 is empty
    rows, first, q, ids, item_row, item_len = case
    none = _run(dev, rows, first, q, ids, item_row[:0], item_len[:0], ratios, top=64)
    assert [o.shape for o in none] == [(0, 64)] * 5
    none = _run(dev, rows, first, q, ids, item_row[:0], item_len[:0], ratios, top=64, max_len=12)
    assert [o.shape for o in none] == [(0, 64)] * 5


def test_a_fast_recording_is_found_along_its_slope_and_not_on_a_diagonal(dev):
    """Uncorrelated unit rows, 3 tracks of 300 / 400 / 350 rows, k = 20: the query is the track's own rows at
    p0 + w(s), 94 of them at num = 266 (+4 %).  Along the slope every row is exact; one diagonal holds at most 26 of
    the 94 rows (w(s) - s is constant over at most 26 consecutive s), so the dense entry scores about 26 / 94 = 0.277
    plus the mean of 68 dot products of unrelated unit vectors (standard deviation 1 / sqrt(128) each)."""
    rng = np.random.RandomState(5)
    first = np.array([0, 300, 700, 1050], np.int64)
    rows = rng.randn(1050, 128).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    ratios = list(range(240, 273, 2))
    truth = [(0, 40), (1, 250), (2, 0), (1, 7)]
    s = np.arange(94)
    at = w(s, 266)
    assert max(np.bincount(at - s)) <= 26
    q = np.concatenate([rows[first[t] + p0 + at] for t, p0 in truth])
    item_row = 94 * np.arange(len(truth), dtype=np.int64)
    item_len = np.full(len(truth), 94, np.int32)
    index = ops.FlatL2Index(device=dev)
    index.add(torch.from_numpy(rows).to(dev))
    ids = index.search(torch.from_numpy(q).to(dev), 20)[1].cpu().numpy()
    tr, off, sc, vo, ra = _run(dev, rows, first, q, ids, item_row, item_len, ratios, top=3)
    dense = _dense(dev, rows, first, q, ids, item_row, item_len, top=3, min_overlap=None)
    for i, (t, p0) in enumerate(truth):
        print(f"track {t} from row {p0}: sloped {sc[i, 0]:.4f} ({vo[i, 0]} votes, ratio {ra[i, 0]}), "
              f"dense {dense[2][i, 0]:.4f} ({dense[3][i, 0]} votes, offset {dense[1][i, 0]})")
        assert (tr[i, 0], off[i, 0], ra[i, 0], vo[i, 0]) == (t, p0, 266, 94), i
        assert abs(float(sc[i, 0]) - 1.0) <= 1e-5
        assert dense[2][i, 0] < 0.5


# ---- the library end to end ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(dev):
    """test_gpu_identify_thin.py's small recipe: an untrained model, 8 tracks of 84 segment hops; the dense f32 library."""
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    tracks = synth_tracks(8, 84 * SEG_HOP / 16000, 4242, dev)
    names = [f"song{i}" for i in range(8)]
    dense = FingerprintLibrary.build(model, list(tracks), cfg, names=names, precision="f32", max_segments=200)
    return cfg, model, tracks, names, dense


@pytest.mark.parametrize("rho", [0.96, 1.0, 1.05])
def test_identify_with_tempo_is_the_restatement_on_its_rows(small, dev, rho):
    """Crops handed over with fs = round(16000 * rho): the device resampler then stretches them, so the recording plays
    the track rho times as fast (tempo and pitch move together)."""
    cfg, model, tracks, names, lib = small
    fs = int(round(16000 * rho))
    queries = [tracks[i % 8, 3000 * i:3000 * i + 56000] for i in range(10)]
    res = lib.identify(queries, fs=fs, top=5, tempo=0.06)
    plain = lib.identify(queries, fs=fs, top=5)
    waves = lib._load_queries(queries, fs)
    segs = [lib.segments(x) for x in waves]
    lens = np.array([s.shape[0] for s in segs], np.int32)
    item_row = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    q = lib._embed(torch.cat(segs, dim=0))
    _, ids = lib.index.search(q, 20)
    ratios = tempo_ratios(0.06, int(lens.max()))
    wt, wo, ws, wv, wr = tempo_ref(lib.rows().cpu().numpy(), lib.first, q.cpu().numpy(), ids.cpu().numpy(), item_row,
                                   lens, ratios, top=5)
    for i, r in enumerate(res):
        assert len(r) == int((wt[i] >= 0).sum()) and r, i
        for j, m in enumerate(r):
            assert (m["track"], m["offset"], m["votes"], m["tempo_num"]) == \
                (int(wt[i, j]), int(wo[i, j]), int(wv[i, j]), int(wr[i, j])), (i, j, m)
            assert abs(m["score"] - float(ws[i, j])) <= 1e-6, (i, j, m, float(ws[i, j]))
            assert m["offset_s"] == m["offset"] * SEG_HOP / 16000 and m["name"] == names[m["track"]]
            assert m["tempo"] == m["tempo_num"] / 256
        # 256 is in the set and the per-track best is a maximum over the ratios
        assert plain[i] and r[0]["score"] >= plain[i][0]["score"], (i, r[0], plain[i][0])
    print(f"rho={rho}: top-1 tempo {[m[0]['tempo_num'] for m in res]}, "
          f"score {np.mean([m[0]['score'] for m in res]):.4f} against {np.mean([m[0]['score'] for m in plain]):.4f}")
    # without tempo nothing changes: the launch is ops.identify on the same rows and ids, bit for bit
    assert lib.identify(queries, fs=fs, top=5, tempo=None) == plain
    t = lambda a: torch.from_numpy(a).to(dev)
    dt, do, ds, dv = (o.cpu().numpy() for o in ops.identify(lib.rows(), t(lib.first), q, ids, t(item_row), t(lens),
                                                            top=5))
    for i, r in enumerate(plain):
        assert [(m["track"], m["offset"], m["score"], m["votes"]) for m in r] == \
            [(int(a), int(b), float(c), int(d)) for a, b, c, d in zip(dt[i], do[i], ds[i], dv[i]) if a >= 0], i
        assert all("tempo" not in m for m in r)


def test_windows_and_timeline_with_tempo(small, dev):
    cfg, model, tracks, names, lib = small
    windows = lib.identify_windows(tracks[2], window_s=3.0, hop_s=1.0, fs=16640, tempo=0.06)
    assert windows and all(wd["matches"] and "tempo" in wd["matches"][0] for wd in windows)
    plain = lib.identify_windows(tracks[2], window_s=3.0, hop_s=1.0, fs=16640)
    assert [wd["segment_start_s"] for wd in windows] == [wd["segment_start_s"] for wd in plain]
    assert all(a["matches"][0]["score"] >= b["matches"][0]["score"] for a, b in zip(windows, plain))
    spans = lib.timeline(windows)
    assert spans and all("tempo" in s and 0.94 <= s["tempo"] <= 1.06 for s in spans)
    assert lib.timeline(plain) == lib.timeline(lib.identify_windows(tracks[2], window_s=3.0, hop_s=1.0, fs=16640,
                                                                    tempo=None))


def test_a_compact_and_a_thinned_library_refuse_tempo(small, dev):
    cfg, model, tracks, names, lib = small
    for other in (lib.thin(2), lib.compress(nlist=4, pq_m=16)):
        with pytest.raises(NotImplementedError, match="tempo"):
            other.identify(tracks[0, :48000], tempo=0.06)
        with pytest.raises(NotImplementedError, match="tempo"):
            other.identify_windows(tracks[0], tempo=0.06)
        assert other.identify(tracks[0, :48000])                                # without it they work as before


@pytest.fixture(scope="module")
def trained(dev):
    """The briefly trained model of _retrieval_case.build_case and its 24 database tracks (seed 1000 + 0)."""
    case = build_case(dev)
    return case["cfg"], case["model"], synth_tracks(24, 20, 1000, dev)


@pytest.mark.statistical
def test_top1_of_a_trained_model_with_and_without_tempo_at_10db(trained, dev):
    """60 crops of 9 s per speed at random sample offsets, white noise at 10 dB SNR, handed over with
    fs = round(16000 * rho) so that the device resampler changes their speed (and their pitch with it: at 4 % that is
    0.7 semitone, which the embedding itself has to survive -- a property of the model, not of the alignment).  Gated
    only on what holds for any model: 256 is among the ratios and a track's best is a maximum over them, so the top-1
    score with tempo is never below the one without.  The figures are printed; measured on MI355X (DESIGN.md section
    12.22), top-1 accuracy dense / tempo and mean top-1 score dense / tempo: rho 0.96: 0.517 / 0.533, 0.636 / 0.643;
    rho 1.0: 1.000 / 1.000, 0.919 / 0.919; rho 1.04: 0.550 / 0.550, 0.686 / 0.694."""
    cfg, model, tracks = trained
    lib = FingerprintLibrary.build(model, list(tracks), cfg)
    rng = np.random.RandomState(23)
    L = 9 * 16000 + 512
    for rho in (0.96, 1.0, 1.04):
        crops, truth = [], []
        for i in range(60):
            t = int(rng.randint(0, 24))
            s0 = int(rng.randint(0, tracks.shape[1] - L))
            crops.append(tracks[t, s0:s0 + L])
            truth.append(t)
        noisy = list(add_noise(torch.stack(crops), 10.0, 41))
        fs = int(round(16000 * rho))
        plain = lib.identify(noisy, fs=fs)
        sloped = lib.identify(noisy, fs=fs, tempo=0.06)
        acc = [float(np.mean([bool(r) and r[0]["track"] == t for r, t in zip(res, truth)])) for res in (plain, sloped)]
        score = [float(np.mean([r[0]["score"] for r in res if r])) for res in (plain, sloped)]
        nums = np.array([r[0]["tempo_num"] for r in sloped if r])
        print(f"rho={rho}: top-1 accuracy dense {acc[0]:.3f} tempo {acc[1]:.3f}; mean top-1 score dense {score[0]:.4f} "
              f"tempo {score[1]:.4f}; winning ratio mean {nums.mean():.1f} (true {256 * rho:.1f}), "
              f"min {nums.min()} max {nums.max()}")
        for p, s in zip(plain, sloped):
            assert not p or (s and s[0]["score"] >= p[0]["score"]), (rho, p[:1], s[:1])
