"""Identification from every Q-th segment of the recording, on the MI355X: grafp_identify_stride_f32 against the numpy
restatement of its contract (tests/_identify_tempo_ref.py at the single ratio 256 * Q, where w(s) = s * Q), against
grafp_identify_f32 at Q = 1 and grafp_identify_tempo_f32 at Q = 2, and query_stride end to end: identify,
identify_windows, the sharded library, StreamMonitor and a briefly trained model at 10 dB SNR."""
import numpy as np
import pytest
import torch

from _identify_tempo_ref import tempo_case, tempo_ref
from _retrieval_case import add_noise, build_case, synth_tracks
from grafp_amd import ops
from grafp_amd.library import FingerprintLibrary, kept_items, window_items
from grafp_amd.monitor import StreamMonitor
from grafp_amd.sharded import ShardedFingerprintLibrary
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
NAMES = ("track", "offset", "score", "votes")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, rows, first, q, ids, item_row, item_len, Q, top, min_overlap=None, max_len=None):
    t = lambda a: torch.from_numpy(a).to(dev)
    out = ops.identify_stride(t(rows), t(first), t(q), t(ids), t(item_row), t(item_len), Q, top=top,
                              min_overlap=min_overlap, max_len=max_len)
    return [o.cpu().numpy() for o in out]


def _ref(rows, first, q, ids, item_row, item_len, Q, top, min_overlap=None):
    return tempo_ref(rows, first, q, ids, item_row, item_len, [256 * Q], top=top, min_overlap=min_overlap)[:4]


def _same_bits(got, want):
    return all(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
               for a, b in zip(got, want))


@pytest.mark.parametrize("min_overlap", [None, 1, 3])
@pytest.mark.parametrize("Q,max_ql", [(2, 40), (3, 20), (4, 16), (8, 8), (32, 3)])
def test_kernel_matches_restatement_bit_exactly_on_dyadic_inputs(dev, Q, max_ql, min_overlap):
    rows, first, q, ids, item_row, item_len = tempo_case(1 + (min_overlap or 0) + 10 * Q, [256 * Q], 64, max_ql, 6)
    got = _run(dev, rows, first, q, ids, item_row, item_len, Q, top=8, min_overlap=min_overlap)
    want = _ref(rows, first, q, ids, item_row, item_len, Q, top=8, min_overlap=min_overlap)
    found = int((got[0][:, 0] >= 0).sum())
    print(f"Q={Q} max_ql={max_ql} min_overlap={min_overlap}: {found} of 64 items find something")
    for g, x, name in zip(got, want, NAMES):
        assert np.array_equal(g, x), (name, np.argwhere(g != x)[:5])
    assert found > 40                                        # most items found something
    # the empty item's padding
    assert item_len[0] == 0 and (got[0][0] == -1).all() and (got[1][0] == np.iinfo(np.int32).min).all()
    assert np.isneginf(got[2][0]).all() and (got[3][0] == 0).all()
    # the same launch with max_len given (asynchronous path)
    again = _run(dev, rows, first, q, ids, item_row, item_len, Q, top=8, min_overlap=min_overlap,
                 max_len=int(item_len.max()))
    assert _same_bits(again, got)


@pytest.mark.parametrize("min_overlap", [None, 1, 3])
def test_stride_one_is_the_dense_kernel_and_stride_two_the_tempo_kernel_at_512(dev, min_overlap):
    t = lambda a: torch.from_numpy(a).to(dev)
    rows, first, q, ids, item_row, item_len = tempo_case(3 + (min_overlap or 0), [256], 64, 40, 6)
    got = _run(dev, rows, first, q, ids, item_row, item_len, 1, top=8, min_overlap=min_overlap)
    dense = ops.identify(t(rows), t(first), t(q), t(ids), t(item_row), t(item_len), top=8, min_overlap=min_overlap)
    assert _same_bits(got, [o.cpu().numpy() for o in dense]) and (got[0][:, 0] >= 0).sum() > 40
    rows, first, q, ids, item_row, item_len = tempo_case(4 + (min_overlap or 0), [512], 64, 40, 6)
    got = _run(dev, rows, first, q, ids, item_row, item_len, 2, top=8, min_overlap=min_overlap)
    sloped = ops.identify_tempo(t(rows), t(first), t(q), t(ids), t(item_row), t(item_len), [512], top=8,
                                min_overlap=min_overlap)
    assert _same_bits(got, [o.cpu().numpy() for o in sloped[:4]]) and (got[0][:, 0] >= 0).sum() > 40


def test_kernel_matches_restatement_at_the_size_limits(dev):
    """256 kept rows with k = 32 (8192 keys: the query rows no longer fit the LDS next to the slots and are read from
    global memory) next to items of 5 and 200 rows in the same launch, Q = 3, over tracks long enough for long runs."""
    Q = 3
    first = np.array([0, 900, 940, 1640], np.int64)
    n = int(first[-1])
    rng = np.random.RandomState(8)
    rows = (rng.randint(-16, 16, size=(n, 128)) / 256.0).astype(np.float32)
    item_len = np.array([256, 5, 200], np.int32)
    item_row = np.array([0, 256, 261], np.int64)
    nq = 461
    q = (rng.randint(-16, 16, size=(nq, 128)) / 256.0).astype(np.float32)
    ids = rng.randint(-1, n, size=(nq, 32)).astype(np.int64)
    ids[:, 5] = (np.arange(nq) * 3) % n                      # long runs of one alignment
    for mo in (None, 1):
        got = _run(dev, rows, first, q, ids, item_row, item_len, Q, top=16, min_overlap=mo)
        want = _ref(rows, first, q, ids, item_row, item_len, Q, top=16, min_overlap=mo)
        for g, x, name in zip(got, want, NAMES):
            assert np.array_equal(g, x), (mo, name, np.argwhere(g != x)[:5])
        assert (got[0][:, 0] >= 0).all()


# ---- the library end to end ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(dev):
    """test_gpu_identify.py's small_lib recipe: an untrained model, 8 tracks of 84 segment hops; the dense library."""
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    tracks = synth_tracks(8, 84 * SEG_HOP / 16000, 4242, dev)
    lib = FingerprintLibrary.build(model, list(tracks), cfg, names=[f"song{i}" for i in range(8)], max_segments=200)
    return cfg, model, tracks, lib


@pytest.mark.parametrize("Q", [2, 4])
def test_clean_grid_crops_are_identified(small, dev, Q):
    """The crops of test_gpu_identify.py's dense test, with its bounds: the pairs of the true alignment are a subset of
    the exact row pairs the dense call scores."""
    cfg, model, tracks, lib = small
    rng = np.random.RandomState(11)
    crops, truth = [], []
    for i in range(40):
        t = i % 8
        L = int(rng.randint(3 * 16000, 5 * 16000))
        j = rng.randint(0, (tracks.shape[1] - L) // SEG_HOP + 1)
        crops.append(tracks[t, j * SEG_HOP:j * SEG_HOP + L])
        truth.append((t, j))
    crops.append(tracks[0, :3000])                                      # shorter than one segment
    res = lib.identify(crops, query_stride=Q)
    assert res[-1] == []
    for (t, j), r in zip(truth, res[:-1]):
        assert r and r[0]["track"] == t and r[0]["name"] == f"song{t}", (t, j, r[:2])
        assert abs(r[0]["offset"] - j) <= 1, (t, j, r[0])
        assert r[0]["offset_s"] == r[0]["offset"] * SEG_HOP / 16000
    assert lib.identify(crops[0], query_stride=Q)[0]["track"] == truth[0][0]    # one waveform in -> one list out
    assert lib.identify(crops[:5], query_stride=1) == lib.identify(crops[:5])


def test_a_recording_longer_than_256_segments(small, dev):
    """60 s are 615 segments: refused at stride 1 with the message of the 256-segment limit, 154 kept rows at stride 4."""
    cfg, model, tracks, lib = small
    long_tracks = synth_tracks(2, 62.0, 77, dev)
    lib2 = FingerprintLibrary.build(model, list(long_tracks), cfg, max_segments=700)
    rec = long_tracks[1, 9 * SEG_HOP:9 * SEG_HOP + 60 * 16000]
    with pytest.raises(ValueError, match="identify_windows for long recordings"):
        lib2.identify(rec)
    res = lib2.identify(rec, query_stride=4)
    assert lib2.segments(rec).shape[0] == 615
    assert res and res[0]["track"] == 1 and abs(res[0]["offset"] - 9) <= 1, res[:2]
    assert res[0]["offset_s"] == res[0]["offset"] * SEG_HOP / 16000


@pytest.fixture(scope="module")
def trained(dev):
    """The briefly trained model of _retrieval_case.build_case and its 24 database tracks (seed 1000 + 0)."""
    case = build_case(dev)
    return case["cfg"], case["model"], synth_tracks(24, 20, 1000, dev)


@pytest.mark.parametrize("Q", [2, 4])
def test_windows_and_timeline(trained, dev, Q):
    """test_gpu_identify.py's recording of three library tracks back to back, a 3 s window every second."""
    cfg, model, tracks = trained
    tracks = tracks[:8, :84 * SEG_HOP]                               # 8.06 s each: a whole number of segment hops
    lib = FingerprintLibrary.build(model, list(tracks), cfg, max_segments=200)
    order = [5, 2, 7]
    rec = torch.cat([tracks[t] for t in order])
    dense = lib.identify_windows(rec, window_s=3.0, hop_s=1.0)
    windows = lib.identify_windows(rec, window_s=3.0, hop_s=1.0, query_stride=Q)
    assert [(x["start_s"], x["end_s"]) for x in windows] == [(x["start_s"], x["end_s"]) for x in dense]
    assert [s["track"] for s in lib.timeline(dense, min_score=0.9)] == order
    spans = lib.timeline(windows, min_score=0.9)
    assert [s["track"] for s in spans] == order, spans
    n_seg = lib.segments(rec).shape[0]
    _, jrow, jlen = window_items(n_seg, rec.numel(), lib.settings, 3.0, 1.0)
    krow, klen = kept_items(jrow, jlen, Q)
    assert (klen > 0).all()
    for x, k, d in zip(windows, krow, dense):
        assert x["segment_start_s"] == int(k) * Q * lib.segment_s     # a multiple of Q segment hops
        assert 0 <= x["segment_start_s"] - d["segment_start_s"] < Q * lib.segment_s


def test_sharded_library_answers_as_one_card(small, dev):
    cfg, model, tracks, lib = small
    sh = ShardedFingerprintLibrary.split(lib, 3)
    queries = [tracks[i % 8, 2000 * i:2000 * i + 50000] for i in range(16)]
    want = lib.identify(queries, query_stride=4)
    assert all(want) and sh.identify(queries, query_stride=4) == want
    rec = torch.cat([tracks[1], tracks[6]])
    assert sh.identify_windows(rec, query_stride=4) == lib.identify_windows(rec, query_stride=4)


# ---- the monitor ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream_case(small, dev):
    """test_gpu_stream.py's stream: 12 s of excerpts of two library tracks, cut from and placed at segment hops."""
    cfg, model, tracks, _ = small
    lib = FingerprintLibrary.build(model, list(tracks[:6]), cfg, names=[f"song{i}" for i in range(6)], precision="f32",
                                   max_segments=200)
    cuts = [(1, 5, 63), (4, 12, 62)]                                  # (track, first segment hop, segment hops)
    stream = torch.cat([tracks[t, j * SEG_HOP:(j + n) * SEG_HOP] for t, j, n in cuts]).contiguous()
    assert stream.numel() == 12 * 16000
    return lib, stream


@pytest.mark.parametrize("Q", [2, 3, 4])
def test_push_rows_reports_the_windows_of_identify_windows(stream_case, dev, Q):
    """The caller's rows stay dense; every row off the channel's grid is NaN here, so one read of such a row would show in
    a score.  The windows agree with identify_windows(query_stride=Q) in every field, however the rows are sliced."""
    lib, stream = stream_case
    want = lib.identify_windows(stream, query_stride=Q)
    kept = lib._embed(lib.segments(stream)[::Q].contiguous())
    rows = torch.full((115, 128), float("nan"), device=dev)
    rows[::Q] = kept
    assert kept.shape[0] == -(-115 // Q) and len(want) == 10 and all(x["matches"] for x in want)
    mon = StreamMonitor(lib, 2, query_stride=Q)
    got, lo = [], 0
    for n in (1, 20, 0, 33, 7, 2, 40, 12):                            # uneven slices; channel 0 stays silent
        out = mon.push_rows([None, rows[lo:lo + n] if n else None])
        assert out[0] == []
        got += out[1]
        lo += n
    assert lo == 115 and 0 < len(got) < len(want)
    got += mon.end(1, n_samples=stream.numel())
    assert [{k: v for k, v in x.items() if k != "channel"} for x in got] == want
    assert all(x["channel"] == 1 for x in got)
    assert mon.timeline(1) == lib.timeline(want)


@pytest.mark.parametrize("Q", [2, 4])
def test_push_of_waveforms_embeds_the_kept_segments_only(stream_case, dev, Q, monkeypatch):
    """1 s chunks on channel 1 of three, the whole stream at once on channel 0: the model is handed ceil(n_seg / Q)
    segments per channel over the stream, and the windows are those of identify_windows(query_stride=Q) -- the same
    items; the scores are not compared, the segments reach the model in other batches."""
    lib, stream = stream_case
    offline = lib.identify_windows(stream, query_stride=Q)
    handed, embed = [], lib._embed
    monkeypatch.setattr(lib, "_embed", lambda segs: handed.append(int(segs.shape[0])) or embed(segs))
    mon = StreamMonitor(lib, 3, max_chunk_s=1.0, query_stride=Q)
    wins = [[], [], []]
    for s in range(12):
        out = mon.push([stream if s == 0 else None, stream[s * 16000:(s + 1) * 16000], None])
        for c in range(3):
            wins[c] += out[c]
    for c, out in enumerate(mon.end([0, 1, 2])):
        wins[c] += out
    assert sum(handed) == 2 * -(-115 // Q)                            # not 2 * 115
    for c in (0, 1):
        assert [(x["start_s"], x["end_s"], x["segment_start_s"], x["channel"]) for x in wins[c]] == \
            [(x["start_s"], x["end_s"], x["segment_start_s"], c) for x in offline]
        for x in wins[c]:
            if 3.0 < x["start_s"] < 7.0:                              # (across the cut: no true alignment)
                continue
            # inside one excerpt (track 1 from its hop 5, then from hop 63 of the stream track 4 from its hop 12): the
            # bounds of test_clean_grid_crops_are_identified, from the window's first KEPT segment
            j0, m = int(round(x["segment_start_s"] / lib.segment_s)), x["matches"][0]
            t, truth = (1, j0 + 5) if x["start_s"] <= 3.0 else (4, j0 - 63 + 12)
            assert j0 % Q == 0 and m["track"] == t and abs(m["offset"] - truth) <= 1, (c, x["start_s"], m, truth)
    assert wins[2] == [{"start_s": 0.0, "end_s": 3.0, "segment_start_s": 0.0, "matches": [], "channel": 2}]


# ---- accuracy -------------------------------------------------------------------------------------------------------
@pytest.mark.statistical
def test_top1_accuracy_of_a_trained_model_at_10db(trained, dev):
    """The 150 three-second queries of test_gpu_identify.py's test of the same name (random sample offsets, white noise
    at 10 dB SNR, the same seeds) through the dense call and through query_stride 2 and 4 in one run.  A strided query
    may lose at most the dense test's own margin at 3 s, 3 queries in 100, against the dense result of this run.
    Measured on MI355X (training is bit-reproducible): dense 1.000, query_stride 2 1.000, query_stride 4 1.000."""
    cfg, model, tracks = trained
    lib = FingerprintLibrary.build(model, list(tracks), cfg)
    rng = np.random.RandomState(21)
    for seconds in (1, 3):                                            # (the 1 s draws come first in that test)
        L = seconds * 16000 + 512
        crops, truth = [], []
        for i in range(150):
            t = int(rng.randint(0, 24))
            s0 = int(rng.randint(0, tracks.shape[1] - L))
            crops.append(tracks[t, s0:s0 + L])
            truth.append(t)
    noisy = list(add_noise(torch.stack(crops), 10.0, 31 + 3))
    acc = {}
    for Q in (1, 2, 4):
        res = lib.identify(noisy, query_stride=Q)
        acc[Q] = float(np.mean([bool(r) and r[0]["track"] == t for r, t in zip(res, truth)]))
    print(f"identify top-1 track accuracy at 10 dB, 3 s: dense {acc[1]:.3f}, query_stride 2 {acc[2]:.3f}, "
          f"query_stride 4 {acc[4]:.3f}")
    assert acc[2] >= acc[1] - 0.03 and acc[4] >= acc[1] - 0.03, acc
