"""Identification against a library that keeps every D-th fingerprint row, on the MI355X: grafp_identify_thin_f32 against
its numpy restatement (tests/_identify_thin_ref.py) and against grafp_identify_f32 at D = 1, and
FingerprintLibrary.build(row_stride=D) / thin(D) end to end (save / load, clean crops, a briefly trained model at
10 dB SNR)."""
import numpy as np
import pytest
import torch

from _identify_thin_ref import thin_case, thin_ref, thin_rows
from _retrieval_case import add_noise, build_case, synth_tracks
from grafp_amd import ops
from grafp_amd.library import FingerprintLibrary
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
NAMES = ("track", "offset", "score", "votes")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, rows, first, q, ids, item_row, item_len, D, top, min_overlap=None, max_len=None):
    t = lambda a: torch.from_numpy(a).to(dev)
    out = ops.identify_thin(t(rows), t(first), t(q), t(ids), t(item_row), t(item_len), D, top=top,
                            min_overlap=min_overlap, max_len=max_len)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("min_overlap", [None, 1, 3])
@pytest.mark.parametrize("D", [1, 2, 3, 5])
def test_kernel_matches_restatement_bit_exactly_on_dyadic_inputs(dev, D, min_overlap):
    rows, first, q, ids, item_row, item_len = thin_case(1 + (min_overlap or 0) + 10 * D, D, 96, 40, 6)
    got = _run(dev, rows, first, q, ids, item_row, item_len, D, top=8, min_overlap=min_overlap)
    want = thin_ref(rows, first, q, ids, item_row, item_len, D, top=8, min_overlap=min_overlap)
    found = int((got[0][:, 0] >= 0).sum())
    print(f"D={D} min_overlap={min_overlap}: {found} of 96 items find something")
    for g, w, name in zip(got, want, NAMES):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])
    assert found > 40                                        # most items found something
    # the same launch with max_len given (asynchronous path)
    again = _run(dev, rows, first, q, ids, item_row, item_len, D, top=8, min_overlap=min_overlap,
                 max_len=int(item_len.max()))
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    if D == 1:                                               # the dense kernel, bit for bit
        t = lambda a: torch.from_numpy(a).to(dev)
        dense = ops.identify(t(rows), t(first), t(q), t(ids), t(item_row), t(item_len), top=8, min_overlap=min_overlap)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(dense, got))


def test_kernel_matches_restatement_at_the_size_limits(dev):
    """ql = 256 with k = 32 (8192 keys: the query rows no longer fit the LDS next to the slots and are read from global
    memory, D rows apart) and a small item in the same launch, D = 4."""
    D = 4
    rows, first, _, _, _, _ = thin_case(7, D, 3, 8, 6)
    n = rows.shape[0]
    item_len = np.array([256, 5, 200], np.int32)
    item_row = np.array([0, 256, 261], np.int64)
    nq = 461
    rng = np.random.RandomState(8)
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = rng.randint(-1, n, size=(nq, 32)).astype(np.int64)
    ids[:, 5] = (np.arange(nq) // D) % n                     # long runs: four alignments, every 4th row of each a hit
    for mo in (None, 1):
        got = _run(dev, rows, first, q, ids, item_row, item_len, D, top=16, min_overlap=mo)
        want = thin_ref(rows, first, q, ids, item_row, item_len, D, top=16, min_overlap=mo)
        for g, w, name in zip(got, want, NAMES):
            assert np.array_equal(g, w), (mo, name, np.argwhere(g != w)[:5])
        assert (got[0][:, 0] >= 0).all()


@pytest.mark.parametrize("D", [2, 5])
def test_kernel_matches_restatement_on_unit_rows_over_200_tracks(dev, D):
    rng = np.random.RandomState(3 + D)
    lens = rng.randint(0, 80, size=200)
    dfirst = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nd = int(dfirst[-1])
    dense = rng.randn(nd, 128).astype(np.float32)
    dense /= np.linalg.norm(dense, axis=1, keepdims=True)
    rows, first = thin_rows(dense, dfirst, D)
    rows = np.ascontiguousarray(rows)
    n_items, k = 300, 10
    item_len = rng.randint(1, 32, size=n_items).astype(np.int32)
    item_row = np.concatenate([[0], np.cumsum(item_len[:-1])]).astype(np.int64)
    q = np.empty((int(item_len.sum()), 128), np.float32)
    for i in range(n_items):
        ql, r0 = int(item_len[i]), int(item_row[i])
        if i % 3 == 2:                                         # a decoy that straddles a track boundary
            t = rng.randint(1, 200)
            a = int(dfirst[t]) - ql // 2
        else:
            t = rng.randint(0, 200)
            a = int(dfirst[t]) + rng.randint(0, max(1, lens[t] - ql + 1))
        src = dense[np.clip(np.arange(a, a + ql), 0, nd - 1)]
        noisy = src + 0.3 * rng.randn(ql, 128).astype(np.float32)
        q[r0:r0 + ql] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
    index = ops.FlatL2Index(device=dev)
    index.add(torch.from_numpy(rows).to(dev))
    _, ids_t = index.search(torch.from_numpy(q).to(dev), k)
    ids = ids_t.cpu().numpy()
    for mo in (None, 4):
        tr, off, sc, vo = _run(dev, rows, first, q, ids, item_row, item_len, D, top=5, min_overlap=mo)
        wt, wo, ws, wv = thin_ref(rows, first, q, ids, item_row, item_len, D, top=5, min_overlap=mo)
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
        print(f"D={D} min_overlap={mo}: {(tr[:, 0] >= 0).mean():.3f} of the items find something")
        assert (tr[:, 0] >= 0).any()


# ---- the library end to end ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(dev):
    """test_gpu_identify.py's small_lib recipe: an untrained model, 8 tracks of 84 segment hops; the dense f32 library."""
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    tracks = synth_tracks(8, 84 * SEG_HOP / 16000, 4242, dev)
    names = [f"song{i}" for i in range(8)]
    dense = FingerprintLibrary.build(model, list(tracks), cfg, names=names, precision="f32", max_segments=200)
    return cfg, model, tracks, names, dense


@pytest.mark.parametrize("D", [2, 5])
def test_build_with_a_row_stride_is_the_thinned_dense_library(small, dev, D):
    cfg, model, tracks, names, dense = small
    built = FingerprintLibrary.build(model, list(tracks), cfg, names=names, precision="f32", max_segments=200,
                                     row_stride=D)
    thin = dense.thin(D)
    assert built.row_stride == thin.row_stride == D and dense.row_stride == 1
    assert built.first.tolist() == thin.first.tolist()
    assert np.diff(built.first).tolist() == [-(-int(v) // D) for v in np.diff(dense.first)]
    err = float((built.rows() - thin.rows()).abs().max())
    print(f"D={D}: rows of build(row_stride) against thin(): max abs difference {err:.2e}")
    assert err <= 1e-4                       # the same segments, packed into other model calls: the f32 embedding bar
    # 772 bytes per kept row, so 772 / D per original row (up to the rounding up of every track's row count)
    assert built.nbytes == 772 * built.n_rows
    # the appended tracks are thinned too
    built.add([tracks[0]], names=["again"])
    assert built.n_tracks == 9 and built.first[-1] - built.first[-2] == built.first[1]


@pytest.mark.parametrize("D", [2, 5])
def test_identify_on_a_thinned_library_is_the_restatement_on_its_rows(small, dev, tmp_path, D):
    cfg, model, tracks, names, dense = small
    lib = FingerprintLibrary.build(model, list(tracks), cfg, names=names, max_segments=200, row_stride=D)
    queries = [tracks[i % 8, 2000 * i:2000 * i + 50000] for i in range(16)]
    res = lib.identify(queries, top=5, min_overlap=None)
    segs = [lib.segments(w) for w in queries]
    lens = np.array([s.shape[0] for s in segs], np.int32)
    item_row = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    q = lib._embed(torch.cat(segs, dim=0))
    _, ids = lib.index.search(q, 20)
    wt, wo, ws, wv = thin_ref(lib.rows().cpu().numpy(), lib.first, q.cpu().numpy(), ids.cpu().numpy(), item_row, lens,
                              D, top=5)
    for i, r in enumerate(res):
        assert len(r) == int((wt[i] >= 0).sum()) and r, i
        for j, m in enumerate(r):
            assert (m["track"], m["offset"], m["votes"]) == (int(wt[i, j]), int(wo[i, j]), int(wv[i, j])), (i, j, m)
            assert abs(m["score"] - float(ws[i, j])) <= 1e-6, (i, j, m, float(ws[i, j]))
            assert m["offset_s"] == m["offset"] * SEG_HOP / 16000 and m["name"] == names[m["track"]]
    # the files: identify is unchanged after load
    lib.save(str(tmp_path / "lib"))
    back = FingerprintLibrary.load(str(tmp_path / "lib"), model)
    assert back.row_stride == D and torch.equal(back.rows(), lib.rows())
    assert back.identify(queries, top=5) == res
    # windows and a timeline go through the same launch
    windows = lib.identify_windows(tracks[2], window_s=3.0, hop_s=1.0)
    assert len(windows) == 6 and all(w["matches"] and w["matches"][0]["track"] == 2 for w in windows)
    assert [s["track"] for s in lib.timeline(windows)] == [2]
    # what needs every row is refused
    with pytest.raises(NotImplementedError, match="row_stride"):
        lib.self_matches()
    with pytest.raises(NotImplementedError, match="row_stride"):
        lib.match(queries[0])
    with pytest.raises(NotImplementedError, match="row_stride"):
        lib.compress()


@pytest.mark.parametrize("D", [2, 5])
def test_clean_grid_crops_are_identified(small, dev, D):
    """The crops of test_gpu_identify.py's dense test, with its bounds: the pairs of the true alignment are exact row
    pairs, the ones the dense library scores too."""
    cfg, model, tracks, names, dense = small
    lib = FingerprintLibrary.build(model, list(tracks), cfg, names=names, max_segments=200, row_stride=D)
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


@pytest.fixture(scope="module")
def trained(dev):
    """The briefly trained model of _retrieval_case.build_case and its 24 database tracks (seed 1000 + 0)."""
    case = build_case(dev)
    return case["cfg"], case["model"], synth_tracks(24, 20, 1000, dev)


@pytest.mark.statistical
@pytest.mark.parametrize("D", [2, 5])
def test_top1_accuracy_of_a_trained_model_at_10db(trained, dev, D):
    """The queries of test_gpu_identify.py's test of the same name (150 per length at random sample offsets, white noise
    at 10 dB SNR) against build(row_stride=D) of the same 24 tracks (bf16).  Measured on MI355X (training is
    bit-reproducible): row_stride 2: 1 s 0.953, 3 s 1.000; row_stride 5: 1 s 0.927, 3 s 1.000; the dense library 0.960 and
    1.000.  A 1 s query is one row: at row_stride 5 the nearest kept row is up to two hops away from it."""
    cfg, model, tracks = trained
    lib = FingerprintLibrary.build(model, list(tracks), cfg, row_stride=D)
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
    print(f"identify top-1 track accuracy at 10 dB, row_stride {D}: 1 s {acc[1]:.3f}, 3 s {acc[3]:.3f} "
          "(dense 0.960 / 1.000)")
    assert acc[1] >= ACC_BAR[D][1] and acc[3] >= ACC_BAR[D][3], acc


# the measured values (0.953 / 1.000 and 0.927 / 1.000) minus the dense test's margins of 4 and 3 queries in 100
ACC_BAR = {2: {1: 0.913, 3: 0.97}, 5: {1: 0.887, 3: 0.97}}
