"""StreamMonitor(tempo=..., tempo_lock=N) on the MI355X (grafp_amd/monitor.py): without a lock
the windows of identify_windows(tempo=...) in every field; with a lock, on rows planted along three slopes, the same
windows however the stream is sliced, those of a window-by-window replay of the rule over ops.identify_tempo
(tests/_stream_tempo_ref.py), and those of a sharded library."""
import numpy as np
import pytest
import torch

from _identify_tempo_ref import tempo_ref
from _retrieval_case import synth_tracks
from _stream_tempo_ref import EXCERPTS, exact_search, planted_library, planted_stream, replay_lock_rule
from grafp_amd import ops
from grafp_amd.library import FingerprintLibrary, window_items
from grafp_amd.monitor import StreamMonitor, samples_lower_bound
from grafp_amd.sharded import ShardedFingerprintLibrary
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
TEMPO, STEP, LOCK = (0.94, 1.06), 4, 3
NUMS = [244, 248, 252, 256, 260, 264, 268]
WINDOW_S, HOP_S, PER_WINDOW = 3.0, 0.5, 21


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def test_without_a_lock_the_windows_are_those_of_identify_windows(dev):
    """test_gpu_stream.py's case: 6 short tracks, an untrained f32 model, the 12 s stream of two excerpts.  push_rows in
    uneven slices and end against identify_windows(tempo=0.06, tempo_step=mon.tempo_step): every field but "channel",
    scores bit for bit (the short windows at the stream's end are searched over the same grid), the same timeline."""
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    tracks = synth_tracks(6, 84 * SEG_HOP / 16000, 4242, dev)
    lib = FingerprintLibrary.build(model, list(tracks), cfg, names=[f"song{i}" for i in range(6)], precision="f32",
                                   max_segments=200)
    stream = torch.cat([tracks[t, j * SEG_HOP:(j + n) * SEG_HOP] for t, j, n in [(1, 5, 63), (4, 12, 62)]]).contiguous()
    mon = StreamMonitor(lib, 2, tempo=0.06)
    assert mon.tempo_step == 12 and mon.tempo_nums.tolist() == [244, 256, 268] and mon.tempo_lock == 0
    want = lib.identify_windows(stream, tempo=0.06, tempo_step=mon.tempo_step)
    rows = lib._embed(lib.segments(stream))
    assert rows.shape[0] == 115 and len(want) == 10 and all(w["matches"] for w in want)
    assert all("tempo_num" in m for w in want for m in w["matches"])
    got, lo = [], 0
    for n in (1, 20, 0, 33, 7, 2, 40, 12):                            # uneven slices; channel 0 stays silent
        out = mon.push_rows([None, rows[lo:lo + n] if n else None])
        assert out[0] == []
        got += out[1]
        lo += n
    assert lo == 115 and 0 < len(got) < len(want)
    got += mon.end(1, n_samples=stream.numel())
    assert [{k: v for k, v in w.items() if k != "channel"} for w in got] == want
    assert all(w["channel"] == 1 and "locked" not in w for w in got)
    assert mon.timeline(1) == lib.timeline(want) and all("tempo" in s for s in mon.timeline(1))
    assert mon.tempo_stats == {"full": 10, "locked": 0, "redone": 0}
    # a finer grid than the windows' own: the monitor passes its step on, so the offline call with it agrees too
    fine = StreamMonitor(lib, 1, tempo=0.06, tempo_step=2)
    got = fine.push_rows([rows])[0] + fine.end(0, n_samples=stream.numel())
    assert [{k: v for k, v in w.items() if k != "channel"} for w in got] == \
        lib.identify_windows(stream, tempo=0.06, tempo_step=2)


def _cpu_replay():
    """The planted library and stream of _stream_tempo_ref.py, the window schedule, and the lock rule replayed on the
    CPU alone (tempo_ref over an exact numpy search).  Windows of 3 s every 0.5 s: 21 rows, a new one every 5.2 rows.

    What the CPU replay must show before anything runs on the GPU -- that the scenario exercises the rule: a locked
    window wholly inside each excerpt; a redone window at each of the two cuts; the planted track on every window wholly
    inside an excerpt, and the planted ratio on at least one of them per excerpt.  NOT the planted ratio on every such
    window: at 264 / 256 the row position w(s) steps ahead of s once every 32 rows, a window of 21 rows holds at most one
    such step, and where it falls inside the window decides which ratio of a grid 4 / 256 apart fits best (a window
    with no step is matched exactly by 256, 260 and 264 and goes to 256, the ratio nearest 1).  Measured with this file's
    seed: excerpt 1 reports 264, 268, 256 ...; that drift of at most one grid step per window is what the lock follows.
    """
    cfg = load_config()
    rows, first = planted_library()
    q, truth = planted_stream(rows, first)
    S = q.shape[0]
    assert S == sum(n for _, _, n, _ in EXCERPTS) == 185
    starts, jrow, lens = window_items(S, samples_lower_bound(S, cfg), cfg, WINDOW_S, HOP_S)
    n_win = int(np.cumprod(lens == PER_WINDOW).sum())               # the windows push_rows reports without end()
    assert n_win == 32
    ids = exact_search(rows, q, 20)
    memo = {}

    def identify(win, sub):
        if (win, tuple(sub)) not in memo:
            r = tempo_ref(rows, first, q, ids, jrow[win:win + 1].astype(np.int64), lens[win:win + 1].astype(np.int32),
                          sub, top=5)
            memo[win, tuple(sub)] = [{"track": int(t), "tempo_num": int(n), "score": float(s)}
                                     for t, n, s in zip(r[0][0], r[4][0], r[2][0]) if t >= 0]
        return memo[win, tuple(sub)]
    ref, stats = replay_lock_rule(identify, n_win, NUMS, LOCK)
    cuts = np.cumsum([n for _, _, n, _ in EXCERPTS])
    for e, (t, num, n, _) in enumerate(EXCERPTS):
        lo, hi = int(cuts[e]) - n, int(cuts[e])
        inside = [w for w in range(n_win) if lo <= jrow[w] and jrow[w] + PER_WINDOW <= hi]
        assert len(inside) >= 4
        assert any(ref[w][1] for w in inside), e                    # a locked window inside the excerpt
        assert all(ref[w][0] and ref[w][0][0]["track"] == t for w in inside), e
        assert any(ref[w][0][0]["tempo_num"] == num for w in inside), e
    redone = [w for w in range(n_win) if ref[w][2]]
    assert len(redone) == stats["redone"] >= 2
    for cut in cuts[:2]:                                             # one at each cut: a window that holds the cut
        assert any(jrow[w] < cut < jrow[w] + PER_WINDOW for w in redone), (cut, [int(jrow[w]) for w in redone])
    assert stats["locked"] >= 3 and stats["full"] + stats["locked"] == n_win
    return cfg, rows, first, q, jrow[:n_win], ref, stats


@pytest.fixture(scope="module")
def planted(dev):
    cfg, rows, first, q, jrow, ref, stats = _cpu_replay()
    lib = FingerprintLibrary(None, cfg, torch.from_numpy(rows).to(dev), first, [f"t{i}" for i in range(6)],
                             precision="f32", device=dev)
    return lib, torch.from_numpy(q).to(dev), jrow, ref, stats


def _monitored(lib, q, step):
    mon = StreamMonitor(lib, 1, window_s=WINDOW_S, hop_s=HOP_S, tempo=TEMPO, tempo_step=STEP, tempo_lock=LOCK)
    assert mon.tempo_nums.tolist() == NUMS
    got = []
    for lo in range(0, q.shape[0], step):
        got += mon.push_rows([q[lo:lo + step]])[0]
    return got, mon.tempo_stats


def test_the_lock_on_planted_rows_is_the_replay_however_the_stream_is_sliced(planted, dev):
    lib, q, jrow, ref, ref_stats = planted
    whole, stats = _monitored(lib, q, q.shape[0])
    assert len(whole) == len(jrow) == 32 and all(list(w)[-1] == "locked" for w in whole)
    for step in (5, 10, 26):
        got, st = _monitored(lib, q, step)
        assert got == whole and st == stats, step
    # the rule replayed window by window over ops.identify_tempo with each window's own ratio sub-list
    ids = lib._search_rows(q, 20)
    first = torch.from_numpy(lib.first).to(dev)

    def identify(win, sub):
        out = ops.identify_tempo(lib.rows(), first, q, ids, torch.tensor([int(jrow[win])], device=dev),
                                 torch.tensor([PER_WINDOW], dtype=torch.int32, device=dev), sub, top=5,
                                 max_len=PER_WINDOW)
        tr, off, sc, vo, ra = (o[0].cpu().numpy() for o in out)
        return [{"track": int(tr[j]), "offset": int(off[j]), "score": float(sc[j]), "votes": int(vo[j]),
                 "tempo_num": int(ra[j])} for j in range(5) if tr[j] >= 0]
    replay, replay_stats = replay_lock_rule(identify, len(jrow), NUMS, LOCK)
    assert stats == replay_stats
    for w, (win, (m, locked, _)) in enumerate(zip(whole, replay)):
        assert win["locked"] == locked, w
        assert [{k: x[k] for k in ("track", "offset", "score", "votes", "tempo_num")} for x in win["matches"]] == m, w
        assert all(x["tempo"] == x["tempo_num"] / 256 and x["name"] == f"t{x['track']}" for x in win["matches"])
    # and what the CPU replay alone promised: the same locks, redone windows, tracks and ratios
    assert stats == ref_stats and stats["redone"] >= 2 and stats["locked"] >= 3
    for w, (win, (m, locked, _)) in enumerate(zip(whole, ref)):
        assert win["locked"] == locked, w
        assert [(x["track"], x["tempo_num"]) for x in win["matches"][:1]] == [(x["track"], x["tempo_num"]) for x in m[:1]]
        assert not m or abs(win["matches"][0]["score"] - m[0]["score"]) <= 1e-5
    print(f"planted stream: {stats}; top-1 (track, num, locked) per window "
          f"{[(x['matches'][0]['track'], x['matches'][0]['tempo_num'], x['locked']) for x in whole]}")


def test_a_sharded_library_reports_the_one_card_windows(planted, dev):
    lib, q, jrow, _, _ = planted
    one, stats = _monitored(lib, q, 26)
    two, stats2 = _monitored(ShardedFingerprintLibrary.split(lib, 2), q, 26)
    assert two == one and stats2 == stats and len(one) == 32
