"""The tempo lock of grafp_amd/monitor.py's StreamMonitor, replayed window by window for ONE channel, and the planted
stream the GPU test feeds.  The rule (the class docstring states it): an unlocked channel's window is searched over the
whole grid, one locked at (t, j) over nums[max(0, j - 1) : j + 2]; a locked search that finds nothing, or another best
track than t, unlocks the channel and the same window is searched again over the whole grid; after the window's final
result no match clears run and lock, else the best match (t', j') extends run if run's last element has track t' and an
index within 1 of j' (otherwise run = [(t', j')]), and once len(run) >= N the lock is (t', j')."""
import numpy as np

from _identify_tempo_ref import w


def replay_lock_rule(identify, n_windows, nums, N):
    """identify(win, sub) -> the matches of window `win` searched over the ratio sub-list `sub`, best first, each a dict
    with at least "track" and "tempo_num" ([]: nothing found).  -> (per window (matches, whether the reported result
    came from the locked search, whether the window was identified twice), {"full", "locked", "redone"} counts)."""
    nums = [int(v) for v in nums]
    R, lock, run = len(nums), None, []
    out, stats = [], {"full": 0, "locked": 0, "redone": 0}
    for win in range(n_windows):
        was_locked, redone = lock is not None, False
        if was_locked:
            m = identify(win, nums[max(0, lock[1] - 1):min(R, lock[1] + 2)])
            if not m or m[0]["track"] != lock[0]:
                lock, run, was_locked, redone = None, [], False, True
                m = identify(win, nums)
                stats["redone"] += 1
        else:
            m = identify(win, nums)
        stats["locked" if was_locked else "full"] += 1
        if not m:
            lock, run = None, []
        else:
            here = (int(m[0]["track"]), nums.index(int(m[0]["tempo_num"])))
            if run and run[-1][0] == here[0] and abs(run[-1][1] - here[1]) <= 1:
                run.append(here)
            else:
                run = [here]
            if len(run) >= N:
                lock = here
        out.append((m, was_locked, redone))
    return out, stats


# the planted stream: (track, num, segments, the track row where the excerpt's first segment sits)
EXCERPTS = ((1, 264, 63, 20), (4, 264, 62, 24), (2, 244, 60, 30))
TRACKS, TRACK_ROWS = 6, 120


def planted_library(seed=11):
    """6 tracks of 120 random unit rows -> (rows (720, 128) f32, first)."""
    rng = np.random.RandomState(seed)
    rows = rng.randn(TRACKS * TRACK_ROWS, 128).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    return rows, TRACK_ROWS * np.arange(TRACKS + 1, dtype=np.int64)


def planted_stream(rows, first):
    """The channel's rows: the library's own, excerpt after excerpt, segment s of an excerpt being the track's row
    p0 + w(s) at the excerpt's ratio -> (stream rows, per segment (track, num))."""
    parts, truth = [], []
    for t, num, n, p0 in EXCERPTS:
        at = int(first[t]) + p0 + w(np.arange(n), num)
        assert at.max() < first[t + 1]
        parts.append(rows[at])
        truth += [(t, num)] * n
    return np.concatenate(parts), truth


def exact_search(rows, q, k):
    """The k nearest library rows of every query row by L2 distance in float64, nearest first -> ids (n, k) int64."""
    d = ((q.astype(np.float64)[:, None, :] - rows.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    return np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int64)
