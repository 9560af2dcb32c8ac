"""Whole recordings against a library on the MI355X: grafp_cross_match_f32 and grafp_cross_match_pq_f32 against their numpy
restatement (tests/_crossmatch_ref.py), bit for bit on all six outputs -- short sources, a source long enough for the
workspace path, partner sorts in the workspace, a short workspace, every PQ width --, against grafp_self_match_f32 on a
library track taken as the source, and FingerprintLibrary.match end to end on both forms of a library (a briefly trained
model on synthetic audio)."""
import numpy as np
import pytest
import torch

from _crossmatch_ref import cross_match_ref, eligible_candidates
from _identify_pq_ref import decode
from _retrieval_case import add_noise, build_case, synth_tracks
from test_gpu_selfmatch import _dyadic_library
from grafp_amd import ops
from grafp_amd._lib import lib
from grafp_amd.library import FingerprintLibrary

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
NAMES = ("track", "delta", "start", "length", "score", "votes")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, rows, first, q, src_first, ids, **kw):
    out = ops.cross_match(_t(dev, rows), _t(dev, first), _t(dev, q), _t(dev, src_first), _t(dev, ids), **kw)
    return [o.cpu().numpy() for o in out]


def _run_pq(dev, pq, first, q, src_first, ids, **kw):
    out = ops.cross_match_pq(*(_t(dev, x) for x in pq), _t(dev, first), _t(dev, q), _t(dev, src_first), _t(dev, ids),
                             **kw)
    return [o.cpu().numpy() for o in out]


def _assert_equal(got, want, tag=""):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        bits = np.uint32 if g.dtype == np.float32 else g.dtype
        same = g.view(bits) == w.view(bits)
        assert same.all(), (tag, name, np.argwhere(~same)[:5], g[~same][:5], w[~same][:5])


def _case(seed, lib_lens, src_lens, k, plants, M=None, p_random=0.3, same_tracks=(), nlist=7):
    """A library of dyadic rows (multiples of 2^-8 in [-1/16, 1/16): random rows, or with M the rows decoded from random
    codes over centroids and codewords in [-1/32, 1/32)) over tracks of the given lengths, built like
    test_gpu_selfmatch._dyadic_library with the source rows kept OUTSIDE it: sources of src_lens random rows; `plants`
    (source, row in it, global library row, length) copy library rows into a source -- across a track boundary too --
    and every planted row hits the row it copies (sometimes twice); the other ids are random, -1 or out of range.
    same_tracks (dst, src): library tracks of equal length with equal rows (equal scores).
    -> (pq or None, rows, first, q, src_first, ids)."""
    rng = np.random.RandomState(seed)
    first = np.concatenate([[0], np.cumsum(lib_lens)]).astype(np.int64)
    n = int(first[-1])
    pq = None
    if M is None:
        rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
        for dst, src in same_tracks:
            rows[first[dst]:first[dst + 1]] = rows[first[src]:first[src + 1]]
    else:
        cent = (rng.randint(-8, 8, size=(nlist, 128)) / 256.0).astype(np.float32)
        books = (rng.randint(-8, 8, size=(M, 256, 128 // M)) / 256.0).astype(np.float32)
        a = rng.randint(0, nlist, size=n).astype(np.int32)
        codes = rng.randint(0, 256, size=(n, M)).astype(np.uint8)
        for dst, src in same_tracks:
            a[first[dst]:first[dst + 1]] = a[first[src]:first[src + 1]]
            codes[first[dst]:first[dst + 1]] = codes[first[src]:first[src + 1]]
        pq = (a, codes, cent, books)
        rows = decode(a, codes, cent, books)
    src_first = np.concatenate([[0], np.cumsum(src_lens)]).astype(np.int64)
    nq = int(src_first[-1])
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = np.where(rng.rand(nq, k) < p_random, rng.randint(0, n, size=(nq, k)), -1).astype(np.int64)
    for s, off, g0, ln in plants:
        q0 = int(src_first[s]) + off
        assert off + ln <= src_lens[s] and g0 + ln <= n, (s, off, g0, ln)
        q[q0:q0 + ln] = rows[g0:g0 + ln]
        for i in range(ln):
            if rng.rand() < 0.9:
                ids[q0 + i, rng.randint(k)] = g0 + i
            if rng.rand() < 0.1:
                ids[q0 + i, rng.randint(k)] = g0 + i                # a duplicate hit, or one that replaces the first
    ids[rng.rand(nq, k) < 0.02] = -5                                 # out of range: no hit
    ids[rng.rand(nq, k) < 0.01] = n + 3
    return pq, rows, first, q, src_first, ids


def _short_case(seed, k, M=None, extra_src=()):
    """About 60 library tracks and 60 sources of 0..70 rows each (zero-row and one-row ones included), 30 planted copies
    at random places, three of them across a track boundary, two library tracks that are equal."""
    rng = np.random.RandomState(seed)
    lib_lens = rng.randint(0, 70, size=60)
    lib_lens[[0, 9, 10]] = 0
    lib_lens[[4, 5]] = 64
    lib_lens[2] = 1
    src_lens = rng.randint(0, 71, size=60)
    src_lens[[0, 7, 59]] = 0
    src_lens[[1, 8]] = 1
    src_lens[[3, 4]] = 70
    src_lens = np.concatenate([src_lens, np.asarray(extra_src, np.int64)]).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(lib_lens)])
    n = int(first[-1])
    plants = [(3, 0, int(first[4]), 64), (4, 6, int(first[5]), 64),            # whole tracks 4 and 5 (equal rows)
              (1, 0, int(first[20]), 1)]
    for t in (12, 30, 44):                                                     # across the end of track t
        plants.append((3 if t == 12 else 4, 0, int(first[t + 1]) - 3, 6))
    for _ in range(30):
        s = int(rng.choice(np.flatnonzero(src_lens >= 8)))
        ln = int(rng.randint(4, min(src_lens[s], 40) + 1))
        plants.append((s, int(rng.randint(0, src_lens[s] - ln + 1)), int(rng.randint(0, n - ln + 1)), ln))
    for j, ln in enumerate(extra_src):                                          # long sources: two long copies
        plants += [(60 + j, 5, int(first[20]), min(ln - 5, 300)), (60 + j, ln // 2, int(first[40]), ln // 2 - 3)]
    return _case(seed + 1, lib_lens, src_lens, k, plants, M=M, same_tracks=[(5, 4)])


@pytest.mark.parametrize("min_votes,min_overlap", [(4, 1), (1, 1), (3, 6)])
@pytest.mark.parametrize("k", [1, 8, 32])
def test_kernel_matches_restatement_bit_exactly_on_many_short_sources(dev, k, min_votes, min_overlap):
    _, rows, first, q, src_first, ids = _short_case(10 + k, k)
    got = _run(dev, rows, first, q, src_first, ids, top=8, min_votes=min_votes, min_overlap=min_overlap)
    want = cross_match_ref(rows, first, q, src_first, ids, top=8, min_votes=min_votes, min_overlap=min_overlap)
    _assert_equal(got, want, (k, min_votes, min_overlap))
    assert (got[0][:, 0] >= 0).sum() >= 20
    for s in (0, 7, 59):                                                        # zero-row sources: padding
        assert (got[0][s] == -1).all() and (got[1][s] == np.iinfo(np.int32).min).all() and (got[2][s] == -1).all()
        assert (got[3][s] == 0).all() and np.isneginf(got[4][s]).all() and (got[5][s] == 0).all()


def test_kernel_matches_restatement_on_a_long_source_through_the_workspace(dev):
    """A 1 100-row source at k = 32 (35 200 hit slots: sorted in four LDS pieces through the workspace) beside a
    520-row one (two pieces), a 40-row one (LDS only) and an empty one."""
    lib_lens = np.array([1200, 300, 0, 600, 40, 64])
    first = np.concatenate([[0], np.cumsum(lib_lens)])
    src_lens = np.array([1100, 520, 40, 0])
    plants = [(0, 0, int(first[1]), 300), (0, 400, int(first[3]), 600), (0, 1000, int(first[1]) + 250, 100),
              (1, 10, 100, 500), (2, 0, int(first[4]), 40), (2, 4, int(first[5]), 30)]
    _, rows, first, q, src_first, ids = _case(3, lib_lens, src_lens, 32, plants, p_random=0.03)
    ids[400:700, 3] = np.arange(int(first[1]), int(first[1]) + 300)             # a second alignment on track 1
    for mv, mo, top in ((4, 1, 8), (1, 1, 64), (2, 20, 4)):
        got = _run(dev, rows, first, q, src_first, ids, top=top, min_votes=mv, min_overlap=mo)
        want = cross_match_ref(rows, first, q, src_first, ids, top=top, min_votes=mv, min_overlap=mo)
        _assert_equal(got, want, (mv, mo))
    assert set(got[0][0, :2]) == {1, 3} and got[0][1, 0] == 0 and got[1][1, 0] == 90 and set(got[0][2, :2]) == {4, 5}


def test_kernel_matches_restatement_when_the_partner_sorts_run_in_the_workspace(dev):
    """More than 16 384 eligible candidates for one source (min_votes = 1): the phase 4-5 key arrays are sorted through
    the workspace.  The construction of test_gpu_selfmatch's test of the same name with the source outside the library:
    a 6 100-row source hits a 6 100-row track at 9 000 distinct offsets, one row each, plus random hits on 40 short
    tracks and a 60-row copy."""
    rng = np.random.RandomState(6)
    lens = np.array([6100] + [20] * 40)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n, k, L = int(first[-1]), 32, 6100
    rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
    q = (rng.randint(-16, 16, size=(L, 128)) / 256.0).astype(np.float32)
    q[2000:2060] = rows[500:560]
    ids = np.full((L, k), -1, np.int64)
    deltas = rng.permutation(np.setdiff1d(np.arange(-6099, 6100), [-1500]))[:9000]     # -1500: the copy's offset
    for c, d in enumerate(deltas):
        i = int(rng.randint(max(0, -d), min(6100, 6100 - d)))
        free = np.flatnonzero(ids[i, :30] < 0)
        if free.size:
            ids[i, free[c % free.size]] = i + d
    ids[:, 30:] = rng.randint(first[1], n, size=(L, 2))                        # the short tracks
    ids[2000:2060, 31] = np.arange(500, 560)                                   # the copy, delta -1500
    src_first = np.array([0, L], np.int64)
    n_elig = len(eligible_candidates(n, first, ids, min_votes=1))
    assert n_elig > 16384, n_elig
    for top in (64, 5):
        got = _run(dev, rows, first, q, src_first, ids, top=top, min_votes=1, min_overlap=1)
        want = cross_match_ref(rows, first, q, src_first, ids, top=top, min_votes=1, min_overlap=1)
        _assert_equal(got, want, top)
    assert got[0][0, 0] == 0 and got[1][0, 0] == -1500 and got[3][0, 0] == 60


def test_sources_past_a_short_workspace_are_marked(dev):
    """A workspace of the header plus the regions of the first sources only (the C entry does not refuse it): every
    source whose region would end past it gets -2 in its first slot; the sources before it are computed as usual."""
    rng = np.random.RandomState(7)
    src_lens = rng.randint(10, 70, size=12)
    src_lens[5] = 0
    lib_lens = rng.randint(10, 70, size=12)
    first = np.concatenate([[0], np.cumsum(lib_lens)])
    plants = [(1, 0, int(first[0]), 10), (4, 2, int(first[3]), 8), (9, 0, int(first[8]), 10)]
    _, rows, first, q, src_first, ids = _case(8, lib_lens, src_lens, 8, plants)
    full = ops.self_match_workspace_bytes(src_lens, 8, 1)
    fits = ops.self_match_workspace_bytes(src_lens[:7], 8, 1)          # 7 and 12 sources share a 256-byte header
    assert fits < full
    ws = torch.zeros(full, dtype=torch.uint8, device=dev)
    outs = [torch.full((12, 8), 7, dtype=torch.float32 if j == 4 else torch.int32, device=dev) for j in range(6)]
    rows_d, first_d, q_d, src_d, ids_d = (_t(dev, x) for x in (rows, first, q, src_first, ids))
    rc = lib.grafp_cross_match_f32(ops._p(rows_d), int(first[-1]), ops._p(first_d), 12, ops._p(q_d), int(src_first[-1]),
                                   ops._p(src_d), 12, ops._p(ids_d), 8, 8, 1, 1, ops._p(ws), fits,
                                   *(ops._p(o) for o in outs), ops._stream())
    assert rc == 0, lib.grafp_last_error()
    got = [o.cpu().numpy() for o in outs]
    want = cross_match_ref(rows, first, q, src_first, ids, top=8, min_votes=1)
    _assert_equal([g[:7] for g in got], [w[:7] for w in want], "fits")
    assert (got[0][7:, 0] == -2).all() and (got[0][7:, 1:] == -1).all() and (got[5][7:] == 0).all()
    assert np.isneginf(got[4][7:]).all() and (ws[fits:] == 0).all()        # nothing written past the given bytes


def test_a_library_track_as_the_source_equals_self_match_on_the_device(dev):
    """ops.cross_match with source = the rows of track a and the hits inside a blanked writes what ops.self_match writes
    for a: a 600-row track at k = 32 (19 200 hit slots: the workspace path), a 40-row one and an empty one."""
    lens = np.array([600, 300, 0, 500, 40])
    rows, first, ids = _dyadic_library(3, lens, 32, [(1, 0, 0, 300), (3, 0, 100, 200), (4, 3, 5, 30)], p_random=0.03)
    rows_d, first_d, ids_d = (_t(dev, x) for x in (rows, first, ids))
    for a in (0, 4, 2):
        fa, fb = int(first[a]), int(first[a + 1])
        own = ids[fa:fb].copy()
        own[(own >= fa) & (own < fb)] = -1
        for mv in (4, 1):
            want = [o.cpu().numpy() for o in ops.self_match(rows_d, first_d, ids_d, tracks=torch.tensor([a]), top=8,
                                                            min_votes=mv)]
            got = _run(dev, rows, first, rows[fa:fb], np.array([0, fb - fa], np.int64), own, top=8, min_votes=mv)
            _assert_equal(got, want, (a, mv))
    assert want[0][0, 0] == -1 and got[0][0, 0] == -1                      # (the empty track: padding from both)


@pytest.mark.parametrize("M", [16, 32, 64, 128])
def test_pq_kernel_matches_restatement_and_the_f32_kernel_bit_exactly(dev, M):
    """Rows decoded from codes (quantisers as tests/test_gpu_identify_pq.py builds them for its bit-exact cases): the
    short-source shape plus a 520-row source (16 640 hit slots at k = 32: two LDS pieces)."""
    pq, rows, first, q, src_first, ids = _short_case(40 + M, 32, M=M, extra_src=[520])
    for mv, mo in ((4, 1), (1, 3)):
        got = _run_pq(dev, pq, first, q, src_first, ids, top=8, min_votes=mv, min_overlap=mo)
        want = cross_match_ref(rows, first, q, src_first, ids, top=8, min_votes=mv, min_overlap=mo)
        _assert_equal(got, want, (M, mv, mo))
        flat = _run(dev, rows, first, q, src_first, ids, top=8, min_votes=mv, min_overlap=mo)
        _assert_equal(got, flat, (M, mv, mo, "f32 kernel"))
    assert (got[0][:, 0] >= 0).sum() >= 20 and got[0][60, 0] >= 0


# ---- the library --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(dev):
    case = build_case(dev)
    return case["cfg"], case["model"], synth_tracks(24, 20, 1000, dev)


def test_medley_copy_and_noise_against_both_forms_of_a_library(trained, dev):
    """A library of 24 tracks (20 s each); a 10 s medley (5 s of track 3, then 5 s of track 7) at 20 dB SNR, an exact
    copy of track 11 and 10 s of white noise, none of them in the library."""
    cfg, model, tracks = trained
    o3, o7 = 40 * SEG_HOP, 70 * SEG_HOP                             # where the medley's pieces start in 3 and 7
    medley = torch.cat([tracks[3, o3:o3 + 5 * 16000], tracks[7, o7:o7 + 5 * 16000]])
    medley = add_noise(medley[None], 20.0, 7)[0]
    noise = torch.randn(10 * 16000, generator=torch.Generator().manual_seed(3)).to(dev) * 0.1
    flat = FingerprintLibrary.build(model, list(tracks), cfg, names=[f"song{i}" for i in range(24)])
    compact = flat.compress(nlist=16, nprobe=8)
    recs = [medley, tracks[11].clone(), noise]
    seg = flat.segment_s
    results = {}
    for form, lib_ in (("flat", flat), ("compact", compact)):
        res = lib_.match(recs)
        assert len(res) == 3
        found = {m["track"]: m for m in res[0]}
        for b, t_in_b, t_in_medley in ((3, o3 / 16000, 0.0), (7, o7 / 16000, 5.0)):
            m = found.get(b)
            assert m is not None, (form, b, res[0])
            want = t_in_b - t_in_medley                               # track time - recording time
            assert abs(m["offset"] * seg - want) <= seg + 1e-6, (form, m, want)
            assert abs((m["track_start_s"] - m["recording_start_s"]) - m["offset"] * seg) <= 1e-9
            # a segment is a window of n_frames * hop_len samples (1.024 s): one that starts less than that before the
            # piece already holds some of it and may vote; 1.5 s (15 segments) are allowed to miss at the piece's start
            seg_len = cfg["n_frames"] * cfg["hop_len"] / cfg["fs"]
            assert max(0.0, t_in_medley - seg_len) - 1e-9 <= m["recording_start_s"] <= t_in_medley + 1.5, (form, m)
            assert 3.0 <= m["overlap_s"] <= 5.0 + seg and m["name"] == f"song{b}", (form, m)
            assert m["recording_coverage"] <= 0.6 and m["track_coverage"] <= 0.3, (form, m)
        assert {res[0][0]["track"], res[0][1]["track"]} == {3, 7}, (form, res[0][:3])
        copy = res[1][0]
        assert copy["track"] == 11 and copy["offset"] == 0 and copy["recording_start_s"] == 0.0, (form, copy)
        assert copy["coverage"] >= 0.99 and copy["track_coverage"] >= 0.99, (form, copy)
        assert lib_.match(recs[1]) == res[1]                          # a single recording: its list alone
        results[form] = (found[3], found[7], copy, res[2])
        print(f"match scores ({form}): copy {copy['score']:.4f}, medley {found[3]['score']:.4f} / "
              f"{found[7]['score']:.4f}, noise recording: " +
              (f"best {res[2][0]['score']:.4f} ({len(res[2])} matches)" if res[2] else "no match"))
    for f, c in zip(results["flat"][:3], results["compact"][:3]):        # the same tracks at the same offsets
        assert (f["track"], f["offset"]) == (c["track"], c["offset"]), (f, c)
    assert flat.n_tracks == 24 and compact.n_tracks == 24                 # nothing was added to either
