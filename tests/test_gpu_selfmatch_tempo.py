"""Tracks that share audio at another speed inside a library, on the MI355X: grafp_self_match_tempo_f32 against its numpy
restatement (tests/_selfmatch_tempo_ref.py), bit for bit on all seven outputs -- short tracks over four ratio sets, the two
identities (ops.self_match at the one ratio 256, ops.cross_match_tempo on the masked hits), a track sorted through the
workspace, partner sorts in the workspace, the merge at its 4096 entries, the empty launches and the short workspace --,
on unit rows gathered along a slope, and FingerprintLibrary.self_matches(tempo=...) end to end (an untrained model, then a
briefly trained one on a library that holds two sped copies of one track)."""
import numpy as np
import pytest
import torch

from _identify_tempo_ref import w
from _retrieval_case import build_case, synth_tracks
from _selfmatch_tempo_ref import (REPEATING, as_cross_match, eligible_of_track, library_case, self_match_tempo_ref,
                                  short_case)
from grafp_amd import ops
from grafp_amd.ops import self_match_tempo          # the op this file is about: without it nothing here can run
from grafp_amd._lib import lib as clib
from grafp_amd.library import DUPLICATE_MIN_SCORE, FingerprintLibrary, tempo_ratios
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
NAMES = ("track", "delta", "start", "length", "score", "votes", "ratio")
RATIO_SETS = {"one": [256], "three": [243, 256, 269], "ends": [128, 256, 512], "all": list(range(225, 289))}
INT_MIN = np.iinfo(np.int32).min


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, rows, first, ids, ratios, tracks=None, **kw):
    out = self_match_tempo(_t(dev, rows), _t(dev, first), _t(dev, ids), ratios, tracks=tracks, **kw)
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
_REF = {}


def _short(which, k):
    """The short case of one ratio set and k, and its restatement per (min_votes, min_overlap): computed once, shared."""
    ratios = RATIO_SETS[which]
    if (which, k) not in _REF:
        _REF[which, k] = (short_case(10 + k + len(ratios), k, ratios), {})
    case, refs = _REF[which, k]

    def ref(min_votes, min_overlap):
        if (min_votes, min_overlap) not in refs:
            refs[min_votes, min_overlap] = self_match_tempo_ref(*case, ratios, top=8, min_votes=min_votes,
                                                                min_overlap=min_overlap)
        return refs[min_votes, min_overlap]
    return case, ratios, ref


@pytest.mark.parametrize("min_votes,min_overlap", [(4, 1), (1, 1), (3, 6)])
@pytest.mark.parametrize("k", [8, 32])
@pytest.mark.parametrize("which", list(RATIO_SETS))
def test_kernel_matches_restatement_bit_exactly_on_many_short_tracks(dev, which, k, min_votes, min_overlap):
    case, ratios, ref = _short(which, k)
    want = ref(min_votes, min_overlap)
    # the conditions hold on the restatement, so the kernel cannot hide behind them
    found = int((want[0][:, 0] >= 0).sum())
    used = sorted(set(want[6][want[0] >= 0].tolist()))
    print(f"{which} k={k} min_votes={min_votes} min_overlap={min_overlap}: {found} of {want[0].shape[0]} tracks find a "
          f"partner, winning ratios {used}")
    assert found >= 15                                                          # more than a handful of sources
    assert len(used) > 1 or len(ratios) == 1                                    # more than one ratio wins somewhere
    for s in (0, 9, 10):                                                        # zero-row tracks: padding
        _assert_padding(want, s)
    assert (want[0] != np.arange(60)[:, None]).all()                            # nobody finds itself
    kw = dict(top=8, min_votes=min_votes, min_overlap=min_overlap)
    _assert_equal(_run(dev, *case, ratios, **kw), want, (which, k, min_votes, min_overlap))
    sub = [41, 9, REPEATING, 3, 0, 5, 59, 17]                                   # a subset, out of order
    _assert_equal(_run(dev, *case, ratios, tracks=torch.tensor(sub), **kw), [x[sub] for x in want], "subset")


# ---- the two identities ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,min_votes,min_overlap", [(8, 4, 1), (8, 3, 6), (32, 1, 1)])
def test_the_ratio_one_is_the_dense_kernel_bit_for_bit(dev, k, min_votes, min_overlap):
    case = short_case(40 + k, k, [256])
    kw = dict(top=8, min_votes=min_votes, min_overlap=min_overlap)
    for tracks in (None, torch.tensor([41, 3, REPEATING, 0, 5])):
        got = self_match_tempo(*(_t(dev, a) for a in case), [256], tracks=tracks, **kw)
        dense = ops.self_match(*(_t(dev, a) for a in case), tracks=tracks, **kw)
        for g, x, name in zip(got, dense, NAMES):
            assert g.dtype == x.dtype and torch.equal(g.view(torch.int32), x.view(torch.int32)), name
        assert torch.equal(got[6], torch.where(got[0] >= 0, 256, 0).to(torch.int32))
    assert int((got[0][:, 0] >= 0).sum()) >= 3


@pytest.mark.parametrize("which", ["three", "ends", "all"])
def test_any_ratios_are_cross_match_tempo_on_the_masked_hits(dev, which):
    ratios = RATIO_SETS[which]
    case = short_case(70 + len(ratios), 8, ratios)
    rows, first, ids = case
    # The track that repeats itself, twice as loud (still dyadic): on itself it scores four times a row's squared norm,
    # against any copy of its rows made before only twice -- with its own-track hits kept it would be its own best match.
    rows[int(first[REPEATING]):int(first[REPEATING + 1])] *= 2
    kw = dict(top=8, min_votes=2, min_overlap=1)
    for tracks in (None, [41, REPEATING, 3, 0, 5]):
        q, src_first, hit = as_cross_match(rows, first, ids, tracks)
        cross = ops.cross_match_tempo(_t(dev, rows), _t(dev, first), _t(dev, q), _t(dev, src_first), _t(dev, hit), ratios,
                                      **kw)
        got = _run(dev, *case, ratios, tracks=None if tracks is None else torch.tensor(tracks), **kw)
        _assert_equal(got, [o.cpu().numpy() for o in cross], (which, tracks))
    # with its own-track hits kept the track that repeats itself would find itself first: the mask matters here
    q, src_first, hit = as_cross_match(rows, first, ids, [REPEATING], mask=False)
    kept = ops.cross_match_tempo(_t(dev, rows), _t(dev, first), _t(dev, q), _t(dev, src_first), _t(dev, hit), ratios, **kw)
    own = _run(dev, *case, ratios, tracks=torch.tensor([REPEATING]), **kw)
    assert int(kept[0][0, 0]) == REPEATING and float(kept[4][0, 0]) > 1.5 * float(own[4][0, 0]) and own[0][0, 0] >= 0
    assert REPEATING not in own[0][0]


# ---- the workspace paths ----------------------------------------------------------------------------------------------
def test_kernel_matches_restatement_on_a_long_track_through_the_workspace(dev):
    """A 520-row track at k = 32 (16 640 hit slots: sorted in two LDS pieces through the workspace) as the second source
    of three, between a 40-row one (LDS only) and a 600-row one, at the ratios 236, 256 and 282: three copies of the
    regions, ratio j's j * total units after ratio 0's."""
    ratios = [236, 256, 282]
    lens = np.array([600, 520, 40, 0, 300])
    first = np.concatenate([[0], np.cumsum(lens)])
    plants = [(1, 10, int(first[0]) + 5, 500, 282), (2, 0, int(first[4]) + 50, 38, 236),
              (0, 50, int(first[4]) + 100, 150, 256), (0, 300, int(first[1]) + 470, 120, 236)]   # the last: across 1's end
    case = library_case(3, lens, 32, plants, p_random=0.03)
    tracks = [2, 1, 0]
    for mv, mo, top in ((4, 1, 8), (1, 1, 64), (2, 20, 4)):
        want = self_match_tempo_ref(*case, ratios, tracks=tracks, top=top, min_votes=mv, min_overlap=mo)
        got = _run(dev, *case, ratios, tracks=torch.tensor(tracks), top=top, min_votes=mv, min_overlap=mo)
        _assert_equal(got, want, (mv, mo, top))
    # what the case is made for, on the restatement: the long plant is a candidate of the 520-row track at its own ratio
    b, a, num, votes, i_lo, m = eligible_of_track(*case, 1, ratios, min_votes=2, min_overlap=20)
    assert ((b == 0) & (num == 282) & (m >= 400)).any()
    assert (want[0][:, 0] >= 0).all() and len(set(want[6][want[0] >= 0].tolist())) >= 2


def test_kernel_matches_restatement_when_the_partner_sorts_run_in_the_workspace(dev):
    """More than 16 384 eligible candidates for one source at each of two ratios (min_votes = 1): the phase 4-5 key
    arrays are sorted through the workspace.  The construction of test_gpu_selfmatch's test of the same name: track 0
    (6 100 rows) hits track 1 (6 100 rows) at 9 000 distinct offsets, one row each, and 40 short tracks at random; a 60-row
    copy of track 1 lies in it along the slope of 262."""
    rng = np.random.RandomState(6)
    ratios = [250, 262]
    lens = np.array([6100, 6100] + [20] * 40)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n, k = int(first[-1]), 32
    rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
    i = np.arange(2000, 2060)
    copy = int(first[1]) + 500 + w(i, 262) - int(w(2000, 262))
    rows[i] = rows[copy]
    ids = np.full((n, k), -1, np.int64)
    deltas = rng.permutation(np.arange(-6099, 6100))[:9000]
    for c, d in enumerate(deltas):
        r = int(rng.randint(max(0, -d), min(6100, 6100 - d)))
        free = np.flatnonzero(ids[r, :30] < 0)
        if free.size:
            ids[r, free[c % free.size]] = first[1] + r + d
    ids[:6100, 30:] = rng.randint(first[2], n, size=(6100, 2))            # the short tracks
    ids[i, 31] = copy                                                     # the copy: a_g = first[1] + 500 - w(2000)
    ids[first[1]:first[2], :4] = rng.randint(first[2], n, size=(6100, 4))   # track 1: on the short tracks
    for num in ratios:
        b, a, _, _, i_lo, m = eligible_of_track(rows, first, ids, 0, [num], min_votes=1)
        assert len(b) > 16384, (num, len(b))
    assert ((b == 1) & (a == int(first[1]) + 500 - int(w(2000, 262))) & (i_lo == 2000) & (m == 60)).sum() == 1
    tracks = [0, 5]
    want = self_match_tempo_ref(rows, first, ids, ratios, tracks=tracks, top=64, min_votes=1, min_overlap=1)
    for top in (64, 5):                                                        # (a shorter list is the longer one's head)
        got = _run(dev, rows, first, ids, ratios, tracks=torch.tensor(tracks), top=top, min_votes=1, min_overlap=1)
        _assert_equal(got, [x[:, :top] for x in want], top)
    assert (want[0][0, :41] >= 0).all() and (want[0][0, 41:] == -1).all() and 1 in want[0][0, :5]


# ---- limits -----------------------------------------------------------------------------------------------------------
def _small_case():
    lens = np.array([30, 0, 25, 40, 12, 33, 1, 20])
    first = np.concatenate([[0], np.cumsum(lens)])
    plants = [(0, 0, int(first[3]) + 2, 20, 230), (0, 4, int(first[5]), 18, 288), (2, 0, int(first[4]), 8, 256),
              (2, 10, int(first[5]), 14, 270), (4, 0, int(first[7]), 10, 225), (5, 2, int(first[3]) + 30, 20, 260)]
    return library_case(77, lens, 6, plants, p_random=0.6)


def test_the_merge_at_its_4096_entries_and_the_empty_launches(dev):
    ratios = list(range(225, 289))
    case = _small_case()
    want = self_match_tempo_ref(*case, ratios, top=64, min_votes=1, min_overlap=1)
    got = _run(dev, *case, ratios, top=64, min_votes=1, min_overlap=1)
    _assert_equal(got, want)
    assert want[0].shape == (8, 64) and (want[0][[0, 2, 4, 5], 0] >= 0).all() and (want[0][:, 8:] == -1).all()
    assert len(set(want[6][want[0] >= 0].tolist())) > 4
    _assert_padding(got, 1)                                                     # a source track of zero rows
    none = _run(dev, *case, ratios, tracks=torch.zeros(0, dtype=torch.int64), top=64)
    assert [o.shape for o in none] == [(0, 64)] * 7 and [o.dtype for o in none] == [x.dtype for x in want]
    empty = _run(dev, *case, ratios, tracks=torch.tensor([1, 1]), top=64)       # zero-row sources alone
    assert [o.shape for o in empty] == [(2, 64)] * 7
    for s in range(2):
        _assert_padding(empty, s)


def test_a_workspace_of_the_header_and_the_lists_alone_gives_padding(dev):
    """Passed straight to the C entry (ops sizes the workspace exactly): ws_bytes holds the header and the lists, which
    the host accepts, but not the regions -- every output is padding and the bytes past ws_bytes are untouched."""
    ratios = [243, 256, 269]
    rows, first, ids = _small_case()
    lens = np.diff(first)
    n_src, top, k = 8, 8, 6
    full = ops.cross_match_tempo_workspace_bytes(lens, k, 1, len(ratios), top)
    given = 256 + 24 * n_src * len(ratios) * top
    assert given < full
    ws = torch.full((full,), 0x5a, dtype=torch.uint8, device=dev)
    outs = [torch.full((n_src, top), 7, dtype=torch.float32 if j == 4 else torch.int32, device=dev) for j in range(7)]
    rows_d, first_d, ids_d = _t(dev, rows), _t(dev, first), _t(dev, ids)
    src = _t(dev, np.arange(n_src, dtype=np.int32))
    nums = (np.array(ratios, np.int32))

    def launch(ws_bytes):
        rc = clib.grafp_self_match_tempo_f32(ops._p(rows_d), int(first[-1]), ops._p(first_d), 8, ops._p(ids_d), k,
                                             ops._p(src), n_src, top, 1, 1, nums.ctypes.data, len(ratios), ops._p(ws),
                                             ws_bytes, *(ops._p(o) for o in outs), ops._stream())
        assert rc == 0, clib.grafp_last_error()
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]

    got = launch(given)
    for s in range(n_src):
        _assert_padding(got, s)
    assert (ws[given:] == 0x5a).all()
    got = launch(full - 8)                                                      # one unit short: still padding, no -2
    for s in range(n_src):
        _assert_padding(got, s)
    assert (ws[full - 8:] == 0x5a).all()
    # the full size computes
    _assert_equal(launch(full), self_match_tempo_ref(rows, first, ids, ratios, top=top, min_votes=1))


# ---- behaviour ------------------------------------------------------------------------------------------------------
def test_a_sped_copy_is_one_match_along_its_slope_and_fragments_on_diagonals(dev):
    """Uncorrelated unit rows, 3 tracks of 900 / 800 / 700 rows, k = 20: track 2 is track 0's rows 30 + w(i) at num = 266
    (+4 %).  Along the slope every row is exact and one candidate holds all 700.  A diagonal holds at most 26 consecutive
    exact rows (w(i) - i steps every 25.6 rows) and min_overlap = 64 asks for spans of 64: whatever the dense kernel finds
    there is at least 38 / 64 uncorrelated rows, so it scores below 26 / 64 + noise < 0.5.  Measured on MI355X: sloped
    (0, 30, 0, 700, 700 votes, 266) at 1.000000; dense best track 0 over 177 rows with 28 votes at 0.1489."""
    rng = np.random.RandomState(5)
    first = np.array([0, 900, 1700, 2400], np.int64)
    rows = rng.randn(2400, 128).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows[first[2]:] = rows[30 + w(np.arange(700), 266)]
    ratios = list(range(240, 273, 2))
    rows_d = torch.from_numpy(rows).to(dev)
    index = ops.FlatL2Index(device=dev)
    index.add(rows_d)
    ids = index.search(rows_d, 20)[1].cpu().numpy()
    b, d, lo, m, sc, vo, ra = _run(dev, rows, first, ids, ratios, top=3, min_votes=4, min_overlap=64)
    dense = [o.cpu().numpy() for o in ops.self_match(rows_d, _t(dev, first), _t(dev, ids), top=3, min_votes=4,
                                                     min_overlap=64)]
    print(f"sloped, track 2: track {b[2, 0]} delta {d[2, 0]} rows {lo[2, 0]}+{m[2, 0]} votes {vo[2, 0]} ratio {ra[2, 0]} "
          f"score {sc[2, 0]:.6f}; track 0: track {b[0, 0]} rows {lo[0, 0]}+{m[0, 0]} ratio {ra[0, 0]} score {sc[0, 0]:.4f}; "
          f"dense best of track 2: track {dense[0][2, 0]} rows {dense[2][2, 0]}+{dense[3][2, 0]} votes {dense[5][2, 0]} "
          f"score {dense[4][2, 0]:.4f}")
    assert (b[2, 0], d[2, 0], lo[2, 0], m[2, 0], vo[2, 0], ra[2, 0]) == (0, 30, 0, 700, 700, 266)
    assert abs(float(sc[2, 0]) - 1.0) <= 1e-5
    # One match with the original.  What else is listed rests on a few of the 20 random hits per row that agree on an
    # alignment: a span of 64 or more uncorrelated unit rows (dot products of sd 0.09) has a mean far below 0.1.
    assert (b[2, 1:] != 0).all() and (sc[2, 1:] < 0.1).all() and (sc[1] < 0.1).all()
    assert float(dense[4][2, 0]) < 0.5


# ---- the library end to end ---------------------------------------------------------------------------------------
def _at_speed(wave, rho):
    """The waveform played rho times as fast (ops.resample from round(16000 * rho) Hz to 16000 Hz)."""
    out, _, lens = ops.resample(wave.contiguous(), [0], [wave.numel()], int(round(16000 * rho)), 16000)
    return out[:int(lens[0])]


@pytest.fixture(scope="module")
def small(dev):
    """test_gpu_identify_thin.py's small recipe (an untrained model, 8 tracks of 84 segment hops, the dense f32 library)
    plus a ninth track: track 3 played at 1.04 times its speed."""
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    tracks = list(synth_tracks(8, 84 * SEG_HOP / 16000, 4242, dev))
    tracks.append(_at_speed(tracks[3], 1.04))
    names = [f"song{i}" for i in range(8)] + ["song3 fast"]
    return FingerprintLibrary.build(model, tracks, cfg, names=names, precision="f32", max_segments=200), names


def test_self_matches_with_tempo_is_the_restatement_on_the_librarys_rows(small, dev):
    lib, names = small
    seg = lib.segment_s
    res = lib.self_matches(tempo=0.06, min_overlap_s=2.0)
    rows = lib.rows()
    _, ids = lib.index.search(rows, 32)
    ratios = tempo_ratios(0.06, 256)
    assert ratios.tolist() == list(range(241, 272))
    min_overlap = int(np.ceil(2.0 / seg - 1e-9))
    wb, wd, wlo, wm, wsc, wvo, wra = self_match_tempo_ref(rows.cpu().numpy(), lib.first, ids.cpu().numpy(), ratios, top=8,
                                                          min_votes=4, min_overlap=min_overlap)
    lens = np.diff(lib.first)
    want = [(a, j) for a in range(9) for j in range(8) if wb[a, j] >= 0]
    assert len(res) == len(want) and res
    for m, (a, j) in zip(res, want):
        b, d, lo, mm, num = int(wb[a, j]), int(wd[a, j]), int(wlo[a, j]), int(wm[a, j]), int(wra[a, j])
        assert (m["track_a"], m["track_b"], m["offset"], m["votes"], m["tempo_num"]) == (a, b, d, int(wvo[a, j]), num)
        assert abs(m["score"] - float(wsc[a, j])) <= 1e-6, (m, float(wsc[a, j]))
        w_lo, w_hi = int(w(lo, num)), int(w(lo + mm - 1, num))
        assert m["name_a"] == names[a] and m["name_b"] == names[b] and m["tempo"] == num / 256
        assert m["a_start_s"] == lo * seg and m["overlap_s"] == mm * seg
        assert m["b_start_s"] == (d + w_lo) * seg and m["b_overlap_s"] == (w_hi - w_lo + 1) * seg
        assert m["coverage"] == max(mm / lens[a], (w_hi - w_lo + 1) / lens[b])
    print("with tempo:", [(m["track_a"], m["track_b"], m["tempo_num"], round(m["overlap_s"] / seg), round(m["score"], 4))
                          for m in res])
    # without tempo: exactly what the dense kernel's outputs gave before this argument existed
    plain = lib.self_matches(min_overlap_s=2.0)
    assert lib.self_matches(min_overlap_s=2.0, tempo=None) == plain
    outs = [o.cpu().numpy() for o in ops.self_match(rows, torch.from_numpy(lib.first).to(dev), ids, top=8, min_votes=4,
                                                    min_overlap=min_overlap)]
    old = [{"track_a": a, "name_a": names[a], "track_b": int(outs[0][a, j]), "name_b": names[int(outs[0][a, j])],
            "offset": int(outs[1][a, j]), "a_start_s": int(outs[2][a, j]) * seg,
            "b_start_s": (int(outs[2][a, j]) + int(outs[1][a, j])) * seg, "overlap_s": int(outs[3][a, j]) * seg,
            "coverage": int(outs[3][a, j]) / max(1, min(int(lens[a]), int(lens[int(outs[0][a, j])]))),
            "score": float(outs[4][a, j]), "votes": int(outs[5][a, j])}
           for a in range(9) for j in range(8) if outs[0][a, j] >= 0]
    assert plain == old and all(list(m) == list(o) for m, o in zip(plain, old))
    print("dense:", [(m["track_a"], m["track_b"], round(m["overlap_s"] / seg), round(m["score"], 4)) for m in plain])
    # 256 is in the grid and a partner's best is a maximum over the ratios
    sloped = {(m["track_a"], m["track_b"]): m["score"] for m in res}
    for m in plain:
        assert sloped[m["track_a"], m["track_b"]] >= m["score"], m


@pytest.fixture(scope="module")
def trained(dev):
    """The briefly trained model of _retrieval_case.build_case and its 24 database tracks (seed 1000 + 0)."""
    case = build_case(dev)
    return case["cfg"], case["model"], synth_tracks(24, 20, 1000, dev)


@pytest.mark.statistical
def test_sped_copies_in_a_library_with_and_without_tempo(trained, dev):
    """The 24 database tracks (20 s each) plus track 3 played at 0.96 (track 24) and at 1.04 (track 25), self-matched with
    and without tempo=0.06 (top = 26: no partner drops off a list's end).  Printed: score and coverage of each sped copy
    against its original, the strongest unrelated pair that passes the 3 s / 4-vote filter, and whether duplicate_groups at
    its default bar joins the copies.  They depend on how far the embedding survives the pitch change, a property of the
    model; gated is only what holds for any model: every score is finite, and a pair found without tempo is found with it
    at a score no lower (256 is among the ratios and a partner's best is a maximum over them).  Measured on MI355X
    (DESIGN.md section 12.26 has the table): the six pairs among tracks 3, 24, 25 score 0.885 to 0.911 dense and 0.894 to
    0.913 with tempo at coverages of 0.17 to 0.28; the strongest unrelated pair 0.8526 both ways; duplicate_groups joins the
    copies neither way, at 0.9 or at 0.8 -- the coverage is what is missing, not the score."""
    cfg, model, tracks = trained
    lib = FingerprintLibrary.build(model, list(tracks) + [_at_speed(tracks[3], 0.96), _at_speed(tracks[3], 1.04)], cfg,
                                   names=[f"song{i}" for i in range(24)] + ["song3 slow", "song3 fast"])
    plain = lib.self_matches(top=26)
    sloped = lib.self_matches(top=26, tempo=0.06)
    related = {(a, b) for a in (3, 24, 25) for b in (3, 24, 25) if a != b}
    for name, res in (("dense", plain), ("tempo", sloped)):
        found = {(m["track_a"], m["track_b"]): m for m in res}
        for pair in sorted(related):
            m = found.get(pair)
            print(f"{name}: {pair} " + ("not found" if m is None else
                  f"score {m['score']:.4f} coverage {m['coverage']:.3f} votes {m['votes']} a {m['a_start_s']:.2f}+"
                  f"{m['overlap_s']:.2f} s" + (f" b +{m['b_overlap_s']:.2f} s ratio {m['tempo_num']}" if "tempo_num" in m
                                               else "")))
        stray = max((m for m in res if (m["track_a"], m["track_b"]) not in related), key=lambda m: m["score"],
                    default=None)
        print(f"{name}: {len(res)} pairs; strongest unrelated pair " + ("none" if stray is None else
              f"({stray['track_a']}, {stray['track_b']}) score {stray['score']:.4f} coverage {stray['coverage']:.3f}"))
        print(f"{name}: duplicate_groups at {DUPLICATE_MIN_SCORE}: {lib.duplicate_groups(res)}; at 0.8: "
              f"{lib.duplicate_groups(res, min_score=0.8)}")
    assert all(np.isfinite(m["score"]) for m in plain + sloped)
    best = {(m["track_a"], m["track_b"]): m["score"] for m in sloped}
    for m in plain:
        pair = (m["track_a"], m["track_b"])
        assert pair in best and best[pair] >= m["score"], (m, best.get(pair))
