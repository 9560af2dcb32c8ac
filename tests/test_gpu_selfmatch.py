"""Shared audio inside a library on the MI355X: grafp_self_match_f32 against its numpy restatement
(tests/_selfmatch_ref.py) -- short tracks, zero-row tracks, a track long enough for the workspace path --, and
FingerprintLibrary.self_matches / duplicate_groups end to end (planted copies in random rows; a briefly trained model on
synthetic audio)."""
import numpy as np
import pytest
import torch

from _retrieval_case import add_noise, build_case, synth_tracks
from _selfmatch_ref import eligible_candidates, self_match_ref
from grafp_amd import ops
from grafp_amd._lib import lib
from grafp_amd.library import DUPLICATE_MIN_SCORE, FingerprintLibrary
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
NAMES = ("track", "delta", "start", "length", "score", "votes")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, rows, first, ids, tracks=None, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = ops.self_match(t(rows), t(first), t(ids), tracks=tracks, **kw)
    return [o.cpu().numpy() for o in out]


def _assert_equal(got, want, tag=""):
    for g, w, name in zip(got, want, NAMES):
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5], g[np.nonzero(g != w)][:5],
                                      w[np.nonzero(g != w)][:5])


def _dyadic_library(seed, lens, k, copies, p_random=0.3):
    """Dyadic rows (multiples of 2^-8 in [-1/16, 1/16)) over tracks of the given lengths; `copies` (dst, src, off, len)
    write rows of one track into another, and every copied row hits its source row (and sometimes twice); the rest of
    the ids are random or -1."""
    rng = np.random.RandomState(seed)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(first[-1])
    rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
    ids = np.where(rng.rand(n, k) < p_random, rng.randint(0, n, size=(n, k)), -1).astype(np.int64)
    for dst, src, off, ln in copies:
        d0, s0 = int(first[dst]) + off, int(first[src])
        rows[d0:d0 + ln] = rows[s0:s0 + ln]
        for i in range(ln):
            if rng.rand() < 0.9:
                ids[d0 + i, rng.randint(k)] = s0 + i
                ids[s0 + i, rng.randint(k)] = d0 + i
            if rng.rand() < 0.1:
                ids[d0 + i, rng.randint(k)] = s0 + i                # a duplicate hit, or one that replaces the first
    ids[rng.rand(n, k) < 0.02] = -5                                  # out of range: no hit
    return rows, first, ids


@pytest.mark.parametrize("min_votes,min_overlap", [(4, 1), (1, 1), (3, 6)])
def test_kernel_matches_restatement_bit_exactly_on_many_short_tracks(dev, min_votes, min_overlap):
    rng = np.random.RandomState(1)
    lens = rng.randint(0, 70, size=60)
    lens[[0, 9, 10]] = 0
    lens[[4, 5, 6, 7]] = 64
    lens[2] = 20
    copies = [(5, 4, 0, 64), (6, 4, 10, 30), (6, 7, 40, 20), (2, 4, 0, 12)]
    rows, first, ids = _dyadic_library(2, lens, 8, copies)
    rows[int(first[7]) + 32:int(first[8])] = rows[int(first[7]):int(first[7]) + 32]   # a track that repeats itself
    got = _run(dev, rows, first, ids, top=8, min_votes=min_votes, min_overlap=min_overlap)
    want = self_match_ref(rows, first, ids, top=8, min_votes=min_votes, min_overlap=min_overlap)
    _assert_equal(got, want)
    assert (got[0][:, 0] >= 0).sum() >= 4
    sub = [9, 6, 0, 5]
    got_s = _run(dev, rows, first, ids, tracks=torch.tensor(sub), top=8, min_votes=min_votes,
                 min_overlap=min_overlap)
    _assert_equal(got_s, [w[sub] for w in want], "subset")


def test_kernel_matches_restatement_on_a_long_track_through_the_workspace(dev):
    """A 6 100-row track at k = 32 (195 200 hit slots: sorted in LDS pieces through the workspace), copies in both
    directions and min_votes = 1 (hundreds of records: the partner sorts still fit in LDS; the next test fills them)."""
    lens = np.array([6100, 300, 0, 500, 40])
    copies = [(1, 0, 0, 300), (3, 0, 100, 200), (4, 3, 5, 30)]
    rows, first, ids = _dyadic_library(3, lens, 32, copies, p_random=0.03)
    ids[1000:1300, 3] = np.arange(int(first[1]), int(first[1]) + 300)           # a second alignment 0 -> 1
    for mv, mo, top in ((4, 1, 8), (1, 1, 64), (2, 20, 4)):
        got = _run(dev, rows, first, ids, top=top, min_votes=mv, min_overlap=mo)
        want = self_match_ref(rows, first, ids, top=top, min_votes=mv, min_overlap=mo)
        _assert_equal(got, want, (mv, mo))
    assert got[0][0, 0] == 1 or got[0][0, 0] == 3


def test_kernel_matches_restatement_when_the_partner_sorts_run_in_the_workspace(dev):
    """More than 16 384 eligible candidates for one source (min_votes = 1): the phase 4-5 key arrays no longer fit in
    LDS and are sorted through the workspace in two pieces, as the hit keys are.  Track 0 (6 100 rows) hits track 1
    (6 100 rows) at 9 000 distinct offsets, one row each, plus random hits on 40 short tracks and a 60-row copy."""
    rng = np.random.RandomState(6)
    lens = np.array([6100, 6100] + [20] * 40)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n, k = int(first[-1]), 32
    rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
    rows[first[1] + 500:first[1] + 560] = rows[2000:2060]
    ids = np.full((n, k), -1, np.int64)
    deltas = rng.permutation(np.setdiff1d(np.arange(-6099, 6100), [-1500]))[:9000]     # -1500: the copy's offset
    for c, d in enumerate(deltas):
        i = int(rng.randint(max(0, -d), min(6100, 6100 - d)))
        free = np.flatnonzero(ids[i, :30] < 0)
        if free.size:
            ids[i, free[c % free.size]] = first[1] + i + d
    ids[:6100, 30:] = rng.randint(first[2], n, size=(6100, 2))            # the short tracks
    ids[2000:2060, 31] = np.arange(first[1] + 500, first[1] + 560)      # the copy, delta -1500
    ids[first[1]:first[2], :4] = rng.randint(first[2], n, size=(6100, 4))   # track 1: on the short tracks
    n_elig = len(eligible_candidates(rows, first, ids, 0, min_votes=1))
    assert n_elig > 16384, n_elig            # else the sorts would stay in LDS (> 8 192) or in one piece (<= 16 384)
    for top in (64, 5):
        got = _run(dev, rows, first, ids, top=top, min_votes=1, min_overlap=1)
        want = self_match_ref(rows, first, ids, top=top, min_votes=1, min_overlap=1)
        _assert_equal(got, want, top)
    assert got[0][0, 0] == 1 and got[1][0, 0] == -1500 and got[3][0, 0] == 60


def test_sources_past_a_short_workspace_are_marked(dev):
    """A workspace of the header plus the regions of the first sources only (the C entry does not refuse it): every
    source whose region would end past it gets -2 in its first slot; the sources before it are computed as usual."""
    rng = np.random.RandomState(7)
    lens = rng.randint(10, 70, size=12)
    lens[5] = 0
    rows, first, ids = _dyadic_library(8, lens, 8, [(1, 0, 0, 10), (4, 3, 2, 8), (9, 8, 0, 10)])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows_d, first_d, ids_d = t(rows), t(first), t(ids)
    src = np.arange(12, dtype=np.int32)
    full = ops.self_match_workspace_bytes(lens, 8, 1)
    fits = ops.self_match_workspace_bytes(lens[:7], 8, 1)          # 7 and 12 sources share a 256-byte header
    assert ops.self_match_workspace_bytes([], 8, 1) == 256 and fits < full
    ws = torch.zeros(full, dtype=torch.uint8, device=dev)
    outs = [torch.full((12, 8), 7, dtype=torch.float32 if j == 4 else torch.int32, device=dev) for j in range(6)]
    rc = lib.grafp_self_match_f32(ops._p(rows_d), int(first[-1]), ops._p(first_d), 12, ops._p(ids_d), 8, ops._p(t(src)),
                                  12, 8, 1, 1, ops._p(ws), fits, *(ops._p(o) for o in outs), ops._stream())
    assert rc == 0, lib.grafp_last_error()
    got = [o.cpu().numpy() for o in outs]
    want = self_match_ref(rows, first, ids, top=8, min_votes=1)
    _assert_equal([g[:7] for g in got], [w[:7] for w in want], "fits")
    assert (got[0][7:, 0] == -2).all() and (got[0][7:, 1:] == -1).all() and (got[5][7:] == 0).all()
    assert np.isneginf(got[4][7:]).all() and (ws[fits:] == 0).all()        # nothing written past the given bytes


def test_kernel_matches_restatement_on_unit_rows_over_200_tracks(dev):
    rng = np.random.RandomState(4)
    lens = rng.randint(0, 90, size=240)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(first[-1])
    rows = rng.randn(n, 128).astype(np.float32)
    planted = []
    for c in range(40):
        src, dst = 2 * c, 2 * c + 1
        ln = min(lens[src], lens[dst], 40)
        if ln < 8:
            continue
        so, do = rng.randint(0, lens[src] - ln + 1), rng.randint(0, lens[dst] - ln + 1)
        rows[first[dst] + do:first[dst] + do + ln] = rows[first[src] + so:first[src] + so + ln] + \
            0.3 * rng.randn(ln, 128).astype(np.float32)
        planted.append((src, dst, do - so))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    index = ops.FlatL2Index(device=dev)
    index.add(torch.from_numpy(rows).to(dev))
    _, ids_t = index.search(torch.from_numpy(rows).to(dev), 16)
    ids = ids_t.cpu().numpy()
    got = _run(dev, rows, first, ids, top=6, min_votes=4)
    want = self_match_ref(rows, first, ids, top=6, min_votes=4)
    for j in (0, 1, 2, 3, 5):
        assert np.array_equal(got[j], want[j]), (NAMES[j], np.argwhere(got[j] != want[j])[:5])
    fin = want[0] >= 0
    assert np.abs(got[4][fin] - want[4][fin]).max() <= 1e-6 and np.isneginf(got[4][~fin]).all()
    for src, dst, d in planted:
        assert got[0][src, 0] == dst and got[1][src, 0] == d, (src, dst, d)
        assert got[0][dst, 0] == src and got[1][dst, 0] == -d, (src, dst, d)


# ---- the library --------------------------------------------------------------------------------------------------
def test_planted_copies_in_a_synthetic_library(dev):
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    rng = np.random.RandomState(5)
    T = 300
    lens = rng.randint(60, 200, size=T)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(first[-1])
    rows = rng.randn(n, 128).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    planted = {}
    for c in range(40):
        src, dst = c, 100 + c
        ln = int(rng.randint(20, 58))
        so, do = rng.randint(0, lens[src] - ln + 1), rng.randint(0, lens[dst] - ln + 1)
        noisy = rows[first[src] + so:first[src] + so + ln] + 0.4 / np.sqrt(128) * rng.randn(ln, 128)
        rows[first[dst] + do:first[dst] + do + ln] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
        planted[(src, dst)] = (do - so, so, ln)
        planted[(dst, src)] = (so - do, do, ln)
    lib = FingerprintLibrary(model, cfg, torch.from_numpy(rows), first, device=dev)
    seg = lib.segment_s
    ms = lib.self_matches(min_overlap_s=1.0, batch_rows=10000)
    found = {(m["track_a"], m["track_b"]): m for m in ms}
    for (a, b), (d, start, ln) in planted.items():
        m = found.get((a, b))
        assert m is not None, (a, b)
        assert m["offset"] == d and abs(m["a_start_s"] / seg - start) <= 1 + 1e-6, (a, b, m, d, start)
        assert abs(m["overlap_s"] / seg - ln) <= 2 + 1e-6 and abs(m["b_start_s"] / seg - (start + d)) <= 1 + 1e-6
        assert m["score"] >= DUPLICATE_MIN_SCORE and m["votes"] >= ln - 2
    stray = [m for m in ms if (m["track_a"], m["track_b"]) not in planted]
    assert all(m["score"] < DUPLICATE_MIN_SCORE for m in stray), stray[:3]
    # a subset of source tracks gives exactly those rows of the full result
    sub = [150, 3, 299, 120]
    want = [m for m in ms if m["track_a"] in sub]
    assert lib.self_matches(min_overlap_s=1.0, tracks=sub) == want


@pytest.fixture(scope="module")
def trained(dev):
    case = build_case(dev)
    return case["cfg"], case["model"], synth_tracks(24, 20, 1000, dev)


def test_medley_and_exact_copy_with_a_trained_model(trained, dev):
    """A library of the 24 database tracks (20 s each), a medley of 5 s of track 3 then 10 s of track 7 at 20 dB SNR,
    and an exact copy of track 11."""
    cfg, model, tracks = trained
    o3, o7 = 40 * SEG_HOP, 70 * SEG_HOP                             # where the medley's pieces start in 3 and 7
    medley = torch.cat([tracks[3, o3:o3 + 5 * 16000], tracks[7, o7:o7 + 10 * 16000]])
    medley = add_noise(medley[None], 20.0, 7)[0]
    lib = FingerprintLibrary.build(model, list(tracks) + [medley, tracks[11].clone()], cfg,
                                   names=[f"song{i}" for i in range(24)] + ["medley", "copy11"])
    seg = lib.segment_s
    ms = lib.self_matches()
    found = {(m["track_a"], m["track_b"]): m for m in ms}
    for b, t_in_b, t_in_medley in ((3, o3 / 16000, 0.0), (7, o7 / 16000, 5.0)):
        for a_, b_, sign in ((24, b, 1), (b, 24, -1)):
            m = found.get((a_, b_))
            assert m is not None, (a_, b_, [x for x in ms if 24 in (x["track_a"], x["track_b"])])
            want = sign * (t_in_b - t_in_medley)                     # track_b time - track_a time
            assert abs(m["offset"] * seg - want) <= seg + 1e-6, (m, want)
            assert abs((m["b_start_s"] - m["a_start_s"]) - want) <= seg + 1e-6, (m, want)
        assert found[(24, b)]["name_a"] == "medley" and found[(24, b)]["name_b"] == f"song{b}"
    assert found[(24, 3)]["overlap_s"] >= 3.0 and found[(24, 7)]["overlap_s"] >= 8.0
    groups = lib.duplicate_groups(ms)
    assert [11, 25] in groups and not any(24 in g for g in groups), groups
    true = {(24, 3), (3, 24), (24, 7), (7, 24), (11, 25), (25, 11)}
    stray = max((m["score"] for m in ms if (m["track_a"], m["track_b"]) not in true), default=float("-inf"))
    print(f"self_matches scores: copy {found[(11, 25)]['score']:.4f} / {found[(25, 11)]['score']:.4f}, medley "
          f"{found[(24, 3)]['score']:.4f} / {found[(24, 7)]['score']:.4f}, strongest unrelated pair {stray:.4f}, "
          f"{len(ms)} pairs")
    assert found[(11, 25)]["coverage"] >= 0.99 and found[(11, 25)]["score"] >= DUPLICATE_MIN_SCORE
    assert stray < DUPLICATE_MIN_SCORE
