"""Whole recordings that play faster or slower than the catalogue, on the MI355X: grafp_cross_match_tempo_f32 against its
numpy restatement (tests/_crossmatch_tempo_ref.py), bit for bit on all seven outputs -- short sources over four ratio sets,
the dense kernel at the one ratio 256, sources sorted through the workspace, partner sorts in the workspace, the merge at
its 4096 entries --, on unit rows planted along a slope, and FingerprintLibrary.match(tempo=...) end to end (an untrained
model, then a briefly trained one on a medley of two speeds)."""
import numpy as np
import pytest
import torch

from _crossmatch_ref import cross_match_ref
from _crossmatch_tempo_ref import cross_match_tempo_ref, eligible_candidates, short_case, tempo_match_case
from _identify_tempo_ref import w
from _retrieval_case import add_noise, build_case, synth_tracks
from grafp_amd import ops
from grafp_amd.library import FingerprintLibrary, tempo_ratios
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
NAMES = ("track", "delta", "start", "length", "score", "votes", "ratio")
RATIO_SETS = {"one": [256], "three": [243, 256, 269], "ends": [128, 256, 512], "nine": list(range(240, 273, 4))}
INT_MIN = np.iinfo(np.int32).min


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, rows, first, q, src_first, ids, ratios, **kw):
    out = ops.cross_match_tempo(_t(dev, rows), _t(dev, first), _t(dev, q), _t(dev, src_first), _t(dev, ids), ratios,
                                **kw)
    return [o.cpu().numpy() for o in out]


def _dense(dev, rows, first, q, src_first, ids, **kw):
    out = ops.cross_match(_t(dev, rows), _t(dev, first), _t(dev, q), _t(dev, src_first), _t(dev, ids), **kw)
    return [o.cpu().numpy() for o in out]


def _assert_equal(got, want, tag=""):
    assert len(got) == len(want)
    for g, x, name in zip(got, want, NAMES):
        assert g.dtype == x.dtype and g.shape == x.shape, (tag, name)
        bits = np.uint32 if g.dtype == np.float32 else g.dtype
        same = g.view(bits) == x.view(bits)
        assert same.all(), (tag, name, np.argwhere(~same)[:5], g[~same][:5], x[~same][:5])


def _assert_padding(out, s):
    assert (out[0][s] == -1).all() and (out[1][s] == INT_MIN).all() and (out[2][s] == -1).all()
    assert (out[3][s] == 0).all() and np.isneginf(out[4][s]).all() and (out[5][s] == 0).all() and (out[6][s] == 0).all()


# ---- the kernel against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("min_votes,min_overlap", [(4, 1), (1, 1), (3, 6)])
@pytest.mark.parametrize("k", [1, 8, 32])
@pytest.mark.parametrize("which", list(RATIO_SETS))
def test_kernel_matches_restatement_bit_exactly_on_many_short_sources(dev, which, k, min_votes, min_overlap):
    ratios = RATIO_SETS[which]
    case = short_case(10 + k + len(ratios), k, ratios)
    want = cross_match_tempo_ref(*case, ratios, top=8, min_votes=min_votes, min_overlap=min_overlap)
    # the conditions hold on the restatement, so the kernel cannot hide behind them
    found = int((want[0][:, 0] >= 0).sum())
    used = sorted(set(want[6][want[0] >= 0].tolist()))
    print(f"{which} k={k} min_votes={min_votes} min_overlap={min_overlap}: {found} of {want[0].shape[0]} sources find "
          f"something, winning ratios {used}")
    assert found >= 20
    assert len(used) > 1 or len(ratios) == 1
    for s in (0, 7, 59):                                                        # zero-row sources: padding
        _assert_padding(want, s)
    got = _run(dev, *case, ratios, top=8, min_votes=min_votes, min_overlap=min_overlap)
    _assert_equal(got, want, (which, k, min_votes, min_overlap))


@pytest.mark.parametrize("k,min_votes,min_overlap", [(1, 1, 1), (8, 4, 1), (8, 3, 6), (32, 1, 1)])
def test_the_ratio_one_is_the_dense_kernel_bit_for_bit(dev, k, min_votes, min_overlap):
    case = short_case(40 + k, k, [256])
    got = _run(dev, *case, [256], top=8, min_votes=min_votes, min_overlap=min_overlap)
    dense = _dense(dev, *case, top=8, min_votes=min_votes, min_overlap=min_overlap)
    _assert_equal(got[:6], dense, (k, min_votes, min_overlap))
    assert np.array_equal(got[6], np.where(got[0] >= 0, 256, 0))
    assert (got[0][:, 0] >= 0).sum() >= 20


def test_kernel_matches_restatement_on_long_sources_through_the_workspace(dev):
    """A 1 100-row source at k = 32 (35 200 hit slots: sorted in four LDS pieces through the workspace) beside a
    520-row one (two pieces), a 40-row one (LDS only) and an empty one, at the ratios 250 and 262 (two distinct copies of
    the regions): plants that do not overlap at both ratios, beyond source row 256, one across a track's end."""
    ratios = [250, 262]
    lib_lens = np.array([1200, 300, 0, 600, 40, 64])
    first = np.concatenate([[0], np.cumsum(lib_lens)])
    src_lens = np.array([1100, 520, 40, 0])
    plants = [(0, 0, int(first[1]), 250, 250), (0, 300, int(first[3]), 500, 262),
              (0, 850, int(first[1]) + 200, 200, 250),                          # across the end of track 1 into track 3
              (1, 10, 100, 500, 262), (2, 0, int(first[4]), 38, 250), (2, 4, int(first[5]), 30, 262)]
    case = tempo_match_case(3, lib_lens, src_lens, 32, plants, p_random=0.03)
    for mv, mo, top in ((4, 1, 8), (1, 1, 64), (2, 20, 4)):
        want = cross_match_tempo_ref(*case, ratios, top=top, min_votes=mv, min_overlap=mo)
        got = _run(dev, *case, ratios, top=top, min_votes=mv, min_overlap=mo)
        _assert_equal(got, want, (mv, mo, top))
    # what the case is made for, on the restatement: the long plants are candidates at their own ratios, one of them ends
    # past source row 256, and the plant across the end of track 1 is a candidate of both of its tracks
    rows, first, q, src_first, ids = case
    b, a, num, votes, i_lo, m = eligible_candidates(len(rows), first, ids[:1100], ratios, min_votes=2, min_overlap=20)
    long = {(int(x), int(y)) for x, y in zip(b[m >= 150], num[m >= 150])}
    assert {(1, 250), (3, 262)} <= long and (i_lo + m)[m >= 150].max() > 700, long
    across = (num == 250) & (i_lo >= 850) & (m >= 40)
    assert {1, 3} <= set(b[across].tolist())
    assert (want[0][[0, 1, 2], 0] >= 0).all() and set(want[6][want[0] >= 0].tolist()) == {250, 262}
    _assert_padding(want, 3)


def test_kernel_matches_restatement_when_the_partner_sorts_run_in_the_workspace(dev):
    """More than 16 384 eligible candidates for one source at each of two ratios (min_votes = 1): the phase 4-5 key
    arrays are sorted through the workspace.  The construction of test_gpu_crossmatch's test of the same name: a
    6 100-row source whose rows hit 40 short tracks at random (spans of at most a short track), a few hundred single rows
    of a 6 100-row track, and a 60-row copy of it along the slope of 262."""
    rng = np.random.RandomState(6)
    ratios = [250, 262]
    lens = np.array([6100] + [20] * 40)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n, k, L = int(first[-1]), 32, 6100
    rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
    q = (rng.randint(-16, 16, size=(L, 128)) / 256.0).astype(np.float32)
    ids = np.full((L, k), -1, np.int64)
    ids[:, :4] = rng.randint(first[1], n, size=(L, 4))                         # the short tracks
    some = rng.choice(L, size=400, replace=False)
    ids[some, 10] = rng.randint(0, 6100, size=400)                             # single rows of the long track
    i = np.arange(2000, 2060)
    copy = 500 + w(i, 262) - int(w(2000, 262))
    q[i] = rows[copy]
    ids[i, 31] = copy                                                          # a = 500 - w(2000)
    src_first = np.array([0, L], np.int64)
    for num in ratios:
        b, a, _, _, i_lo, m = eligible_candidates(n, first, ids, [num], min_votes=1)
        assert len(b) > 16384, (num, len(b))
    assert ((b == 0) & (a == 500 - int(w(2000, 262))) & (i_lo == 2000) & (m == 60)).sum() == 1      # the copy, at 262
    want = cross_match_tempo_ref(rows, first, q, src_first, ids, ratios, top=64, min_votes=1, min_overlap=1)
    for top in (64, 5):                                                        # (a shorter list is the longer one's head)
        got = _run(dev, rows, first, q, src_first, ids, ratios, top=top, min_votes=1, min_overlap=1)
        _assert_equal(got, [x[:, :top] for x in want], top)
    assert (want[0][0, :41] >= 0).all() and (want[0][0, 41:] == -1).all() and 0 in want[0][0, :5]


@pytest.mark.parametrize("k", [2, 4, 16])
def test_equal_scores_of_one_partner_go_to_the_smaller_alignment(dev, k):
    """Every library row and every source row is the same vector, every hit a row of its own: all candidates of a
    partner score the same to the bit (m = 1 mostly), and the rule alone decides -- the ratio nearer to 1, then the
    smaller alignment.  With k = 4 and 16 a source's candidates are found by walkers of more than one wavefront, so the
    order in which they are stored varies from launch to launch; the answer must not.  The dense kernel runs the same
    body and gets the same case."""
    rng = np.random.RandomState(k)
    base = (rng.randint(-16, 16, size=(1, 128)) / 256.0).astype(np.float32)
    rows = np.repeat(base, 4000, axis=0)
    first = np.array([0, 1500, 1500, 4000], np.int64)
    q = np.repeat(base, 50, axis=0)
    src_first = np.array([0, 30, 50], np.int64)
    ids = rng.choice(4000, size=50 * k, replace=False).reshape(50, k).astype(np.int64)
    want = cross_match_ref(rows, first, q, src_first, ids, top=3, min_votes=1, min_overlap=1)
    _assert_equal(_dense(dev, rows, first, q, src_first, ids, top=3, min_votes=1, min_overlap=1), want, ("dense", k))
    assert (want[0][:, :2] == [0, 2]).all() and (want[0][:, 2] == -1).all() and (want[3][:, :2] >= 1).all()
    for ratios in ([256], [250, 262], [128, 256, 512]):
        want = cross_match_tempo_ref(rows, first, q, src_first, ids, ratios, top=3, min_votes=1, min_overlap=1)
        got = _run(dev, rows, first, q, src_first, ids, ratios, top=3, min_votes=1, min_overlap=1)
        _assert_equal(got, want, (k, ratios))
        assert (want[6][:, :2] == (256 if 256 in ratios else 250)).all()


def test_the_merge_at_its_4096_entries_and_the_empty_launches(dev):
    ratios = list(range(225, 289))
    lib_lens = np.array([30, 0, 25, 40, 12, 33, 1, 20])
    first = np.concatenate([[0], np.cumsum(lib_lens)])
    src_lens = np.array([24, 0, 30, 12, 1, 28])
    plants = [(0, 0, int(first[0]) + 2, 20, 230), (0, 4, int(first[3]), 18, 288), (2, 0, int(first[2]), 8, 256),
              (2, 10, int(first[5]), 20, 270), (3, 0, int(first[4]), 10, 225), (5, 2, int(first[3]) + 30, 20, 260)]
    case = tempo_match_case(77, lib_lens, src_lens, 6, plants, p_random=0.6)
    want = cross_match_tempo_ref(*case, ratios, top=64, min_votes=1, min_overlap=1)
    got = _run(dev, *case, ratios, top=64, min_votes=1, min_overlap=1)
    _assert_equal(got, want)
    assert want[0].shape == (6, 64) and (want[0][[0, 2, 3, 5], 0] >= 0).all() and (want[0][:, 8:] == -1).all()
    assert len(set(want[6][want[0] >= 0].tolist())) > 4
    _assert_padding(got, 1)
    rows, first, q, src_first, ids = case
    none = _run(dev, rows, first, q[:0], np.zeros(1, np.int64), ids[:0], ratios, top=64)
    assert [o.shape for o in none] == [(0, 64)] * 7
    empty = _run(dev, rows, first, q[:0], np.zeros(4, np.int64), ids[:0], ratios, top=64)
    assert [o.shape for o in empty] == [(3, 64)] * 7
    for s in range(3):
        _assert_padding(empty, s)


# ---- behaviour ------------------------------------------------------------------------------------------------------
def test_a_fast_recording_is_one_match_along_its_slope_and_fragments_on_diagonals(dev):
    """Uncorrelated unit rows, 3 tracks of 900 / 800 / 700 rows, k = 20: the source is track 1's rows 30 + w(i), 600 of
    them at num = 266 (+4 %).  Along the slope every row is exact and one candidate holds all 600; one diagonal holds at
    most 26 consecutive rows, so the dense best is a fragment (measured on MI355X: 36 rows at 0.7297, as the restatement
    with an exact numpy search gave on the CPU: 36 rows at 0.730)."""
    rng = np.random.RandomState(5)
    first = np.array([0, 900, 1700, 2400], np.int64)
    rows = rng.randn(2400, 128).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    ratios = list(range(240, 273, 2))
    q = rows[first[1] + 30 + w(np.arange(600), 266)]
    src_first = np.array([0, 600], np.int64)
    index = ops.FlatL2Index(device=dev)
    index.add(torch.from_numpy(rows).to(dev))
    ids = index.search(torch.from_numpy(q).to(dev), 20)[1].cpu().numpy()
    b, d, lo, m, sc, vo, ra = _run(dev, rows, first, q, src_first, ids, ratios, top=3, min_votes=4, min_overlap=32)
    dense = _dense(dev, rows, first, q, src_first, ids, top=3, min_votes=4, min_overlap=32)
    print(f"sloped: track {b[0, 0]} delta {d[0, 0]} rows {lo[0, 0]}+{m[0, 0]} votes {vo[0, 0]} ratio {ra[0, 0]} score "
          f"{sc[0, 0]:.6f}; dense best: track {dense[0][0, 0]} delta {dense[1][0, 0]} rows {dense[2][0, 0]}+"
          f"{dense[3][0, 0]} votes {dense[5][0, 0]} score {dense[4][0, 0]:.4f}")
    assert (b[0, 0], d[0, 0], lo[0, 0], m[0, 0], vo[0, 0], ra[0, 0]) == (1, 30, 0, 600, 600, 266)
    assert abs(float(sc[0, 0]) - 1.0) <= 1e-5
    assert dense[3][0, 0] < 100 and dense[4][0, 0] < 0.9


# ---- the library end to end ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(dev):
    """test_gpu_identify_tempo.py's small recipe: an untrained model, 8 tracks of 84 segment hops; the dense f32 library."""
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    tracks = synth_tracks(8, 84 * SEG_HOP / 16000, 4242, dev)
    names = [f"song{i}" for i in range(8)]
    dense = FingerprintLibrary.build(model, list(tracks), cfg, names=names, precision="f32", max_segments=200)
    return cfg, model, tracks, names, dense


@pytest.mark.parametrize("rho", [0.96, 1.0, 1.05])
def test_match_with_tempo_is_the_restatement_on_its_rows(small, dev, rho):
    """Whole tracks and two-track joins handed over with fs = round(16000 * rho): the device resampler then stretches
    them, so the recording plays the tracks rho times as fast."""
    cfg, model, tracks, names, lib = small
    fs = int(round(16000 * rho))
    recs = [tracks[1], tracks[6], torch.cat([tracks[2], tracks[5]]), torch.cat([tracks[7], tracks[0]])]
    res = lib.match(recs, fs=fs, tempo=0.06)
    plain = lib.match(recs, fs=fs)
    assert lib.match(recs, fs=fs, tempo=None) == plain
    assert all("tempo" not in m and len(m) == 11 for r in plain for m in r)
    q, counts = lib._fingerprint_tracks(lib._load_queries(recs, fs), 4096)
    _, ids = lib.index.search(q, 20)
    ratios = tempo_ratios(0.06, 256)
    assert ratios.tolist() == list(range(241, 272))
    src_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    seg = lib.segment_s
    min_overlap = int(np.ceil(3.0 / seg - 1e-9))
    wb, wd, wlo, wm, wsc, wvo, wra = cross_match_tempo_ref(lib.rows().cpu().numpy(), lib.first, q.cpu().numpy(),
                                                           src_first, ids.cpu().numpy(), ratios, top=8, min_votes=4,
                                                           min_overlap=min_overlap)
    lens = np.diff(lib.first)
    for s, r in enumerate(res):
        assert len(r) == int((wb[s] >= 0).sum()) and r, s
        for j, m in enumerate(r):
            b, d, lo, mm, num = int(wb[s, j]), int(wd[s, j]), int(wlo[s, j]), int(wm[s, j]), int(wra[s, j])
            assert (m["track"], m["offset"], m["votes"], m["tempo_num"]) == (b, d, int(wvo[s, j]), num), (s, j, m)
            assert abs(m["score"] - float(wsc[s, j])) <= 1e-6, (s, j, m, float(wsc[s, j]))
            # the derived fields
            w_lo, w_hi = int(w(lo, num)), int(w(lo + mm - 1, num))
            assert m["name"] == names[b] and m["tempo"] == num / 256
            assert m["recording_start_s"] == lo * seg and m["overlap_s"] == mm * seg
            assert m["track_start_s"] == (d + w_lo) * seg and m["track_overlap_s"] == (w_hi - w_lo + 1) * seg
            assert m["recording_coverage"] == mm / counts[s] and m["track_coverage"] == (w_hi - w_lo + 1) / lens[b]
            assert m["coverage"] == max(m["recording_coverage"], m["track_coverage"])
        # 256 is in the grid and a partner's best is a maximum over the ratios
        sloped = {m["track"]: m["score"] for m in r}
        for m in plain[s]:
            assert m["track"] in sloped and sloped[m["track"]] >= m["score"], (s, m, sloped)
    print(f"rho={rho}: top-1 (track, tempo_num, rows, score) {[(r[0]['track'], r[0]['tempo_num'], round(r[0]['overlap_s'] / seg), round(r[0]['score'], 4)) for r in res]}"
          f" against dense {[(r[0]['track'], round(r[0]['overlap_s'] / seg), round(r[0]['score'], 4)) if r else None for r in plain]}")
    # a single recording: its list alone (embedded in a batch of its own, so its rows may differ in their last bits)
    alone = lib.match(recs[0], fs=fs, tempo=0.06)
    assert alone and all(isinstance(m, dict) and list(m) == list(res[0][0]) for m in alone)


@pytest.fixture(scope="module")
def trained(dev):
    """The briefly trained model of _retrieval_case.build_case and its 24 database tracks (seed 1000 + 0)."""
    case = build_case(dev)
    return case["cfg"], case["model"], synth_tracks(24, 20, 1000, dev)


@pytest.mark.statistical
def test_a_medley_of_two_speeds_with_and_without_tempo(trained, dev):
    """A medley of 8 s of track 3 played at 1.04 and 8 s of track 7 played at 0.96 (each resampled on the device), white
    noise at 20 dB SNR, matched with and without tempo=0.06.  Gated only on what holds for any model: every score is
    finite, and a track found without tempo is found with it at a score no lower (256 is in the grid).  The spans, the
    winning ratios and the scores are printed.  Measured on MI355X: dense track 3 at 0.9051
    (13 votes, 3.07 s) and track 7 at 0.7608 (10 votes, 3.07 s); with tempo track 3 at 0.9124 (17 votes, 3.26 s, ratio 265)
    and track 7 at 0.7663 (10 votes, 3.17 s, ratio 241)."""
    cfg, model, tracks = trained
    lib = FingerprintLibrary.build(model, list(tracks), cfg, names=[f"song{i}" for i in range(24)])
    o3, o7 = 40 * SEG_HOP, 70 * SEG_HOP
    fast = lib._load_queries([tracks[3, o3:o3 + int(8 * 16000 * 1.04)]], int(round(16000 * 1.04)))[0]
    slow = lib._load_queries([tracks[7, o7:o7 + int(8 * 16000 * 0.96)]], int(round(16000 * 0.96)))[0]
    medley = add_noise(torch.cat([fast, slow])[None], 20.0, 7)[0]
    plain = lib.match(medley, top=24)                                       # every track: none drops off a list's end
    sloped = lib.match(medley, top=24, tempo=0.06)
    for name, res in (("dense", plain), ("tempo", sloped)):
        for m in res:
            print(f"{name}: track {m['track']} score {m['score']:.4f} votes {m['votes']} recording "
                  f"{m['recording_start_s']:.2f}+{m['overlap_s']:.2f} s track {m['track_start_s']:.2f} s"
                  + (f"+{m['track_overlap_s']:.2f} s ratio {m['tempo_num']}" if "tempo_num" in m else ""))
    assert all(np.isfinite(m["score"]) for m in plain + sloped)
    best = {m["track"]: m["score"] for m in sloped}
    for m in plain:
        assert m["track"] in best and best[m["track"]] >= m["score"], (m, best)
