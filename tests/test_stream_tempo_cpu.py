"""StreamMonitor(tempo=..., tempo_lock=N) without a GPU (grafp_amd/monitor.py): the lock rule on a
library whose _identify_lists hook is scripted -- what a window finds is a table of the test, and the ratio windows the
monitor asks for are recorded -- the refusals, ops.identify_tempo_items' host checks, the C entry and the shipped
assembly.  No GPU call is made."""
import ctypes
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from grafp_amd import library, monitor, ops
from grafp_amd.library import FingerprintLibrary, window_items
from grafp_amd.util import load_config

TEMPO, STEP = (0.94, 1.06), 4
NUMS = [244, 248, 252, 256, 260, 264, 268]
R = len(NUMS)
KEYS = ["start_s", "end_s", "segment_start_s", "matches", "channel"]


class Scripted:
    """A flat CPU library of 6 tracks of 10 rows whose search finds nothing and whose _identify_lists answers from
    script[channel][window] = (track, index into NUMS) or None: the window holds that track at that ratio and nothing
    else, so a search whose ratio window leaves the index out finds nothing.  Channel and segment of a row are written
    into the rows the test pushes.  calls: per launch, the list of (channel, window, lo, cnt)."""

    def __init__(self, script, takes_item_ratios=True):
        cfg = load_config()
        self.lib = FingerprintLibrary(None, cfg, torch.zeros((60, 128)), 10 * np.arange(7), None, precision="f32",
                                      device="cpu")
        self.script, self.calls = script, []
        _, jrow, _ = window_items(2000, 10 ** 8, cfg, 3.0, 1.0)
        self.window_of = {int(j): w for w, j in enumerate(jrow)}
        self.lib._search_rows = lambda q, k: torch.zeros((q.shape[0], 1), dtype=torch.int64)
        if takes_item_ratios:
            self.lib._identify_lists = self.hook
        else:                                                # a fake of the hook written before item_ratios existed
            self.lib._identify_lists = lambda q, ids, item_row, item_len, top, min_overlap, max_len, nums=None, \
                q_stride=1: self.hook(q, ids, item_row, item_len, top, min_overlap, max_len, nums, q_stride)

    def hook(self, q, ids, item_row, item_len, top, min_overlap, max_len, nums=None, q_stride=1, item_ratios=None):
        n = len(item_row)
        tr = torch.full((n, top), -1, dtype=torch.int32)
        off = torch.full((n, top), np.iinfo(np.int32).min, dtype=torch.int32)
        sc = torch.full((n, top), -np.inf)
        vo, ra = torch.zeros((n, top), dtype=torch.int32), torch.zeros((n, top), dtype=torch.int32)
        call = []
        for i in range(n):
            ch, seg = int(q[item_row[i], 1]), int(q[item_row[i], 0])
            win = self.window_of[seg]
            lo, cnt = (0, R) if item_ratios is None else (int(item_ratios[0][i]), int(item_ratios[1][i]))
            call.append((ch, win, lo, cnt) if nums is not None else (ch, win))
            hit = self.script[ch][win] if win < len(self.script[ch]) else None
            if hit is not None and nums is not None and lo <= hit[1] < lo + cnt:
                tr[i, 0], off[i, 0], sc[i, 0], vo[i, 0], ra[i, 0] = hit[0], 2, 0.5 + 0.001 * win, 21, int(nums[hit[1]])
            elif hit is not None and nums is None:
                tr[i, 0], off[i, 0], sc[i, 0], vo[i, 0] = hit[0], 2, 0.5, 21
        assert nums is None or list(nums) == NUMS
        self.calls.append(call)
        return (tr, off, sc, vo, ra) if nums is not None else (tr, off, sc, vo)


def _rows(ch, lo, hi):
    r = torch.zeros((hi - lo, 128))
    r[:, 0] = torch.arange(lo, hi, dtype=torch.float32)
    r[:, 1] = ch
    return r


def _feed(mon, n_rows, step, channels=None):
    """Rows [0, n_rows) of every channel in slices of `step` -> the windows reported per channel."""
    C = mon.channels
    got = [[] for _ in range(C)]
    for lo in range(0, n_rows, step):
        out = mon.push_rows([_rows(ch, lo, min(n_rows, lo + step)) if channels is None or ch in channels else None
                             for ch in range(C)])
        for ch in range(C):
            got[ch] += out[ch]
    return got


def _monitor(script, lock=3, channels=1, **kw):
    fake = Scripted(script)
    return fake, monitor.StreamMonitor(fake.lib, channels, tempo=TEMPO, tempo_step=STEP, tempo_lock=lock, **kw)


def _flat(calls, ch=0):
    return [(w, lo, cnt) for call in calls for c, w, lo, cnt in call if c == ch]


def ROWS_FOR(n_windows):
    """The fewest rows after which push_rows has reported exactly that many whole windows."""
    cfg = load_config()
    for n in range(21, 4000):
        _, _, lens = window_items(n, monitor.samples_lower_bound(n, cfg), cfg, 3.0, 1.0)
        if int(np.cumprod(lens == 21).sum()) == n_windows:
            return n
    raise AssertionError(n_windows)


def test_the_grid_is_fixed_at_construction():
    fake, mon = _monitor([[]])
    assert mon.tempo_nums.tolist() == NUMS and mon.tempo_step == 4 and mon.tempo_lock == 3
    assert mon.tempo_stats == {"full": 0, "locked": 0, "redone": 0}
    auto = monitor.StreamMonitor(fake.lib, 1, tempo=0.06)                        # 21 segments a window: 256 // 21
    assert auto.tempo_step == 12 and auto.tempo_nums.tolist() == library.tempo_ratios(0.06, 21).tolist()
    assert auto.tempo_nums.tolist() == library.tempo_ratios(0.06, 5, auto.tempo_step).tolist()   # short windows too


@pytest.mark.parametrize("N", [1, 3, 4])
def test_the_lock_engages_after_exactly_n_agreeing_windows(N):
    fake, mon = _monitor([[(1, 4)] * 8], lock=N)
    got = _feed(mon, ROWS_FOR(8), 10)[0]
    assert len(got) == 8
    seen = _flat(fake.calls)
    assert seen == [(w, 0, R) if w < N else (w, 3, 3) for w in range(8)]       # window N is the first locked one
    assert [w["locked"] for w in got] == [i >= N for i in range(8)]
    assert mon.tempo_stats == {"full": N, "locked": 8 - N, "redone": 0}
    assert all(w["matches"][0]["tempo_num"] == 260 and w["matches"][0]["track"] == 1 for w in got)
    assert all(list(w) == KEYS + ["locked"] for w in got)


def test_the_window_follows_the_drift_and_is_clipped_at_both_ends():
    js = [4, 4, 4, 5, 6, 6, 5, 4, 3, 2, 1, 0, 0, 1]
    fake, mon = _monitor([[(2, j) for j in js]])
    got = _feed(mon, ROWS_FOR(len(js)), 7)[0]
    seen = _flat(fake.calls)
    want = [(w, 0, R) for w in range(3)]
    for w in range(3, len(js)):
        j = js[w - 1]                                                            # the lock the window before left
        lo = max(0, j - 1)
        want.append((w, lo, min(R, j + 2) - lo))
    assert seen == want and mon.tempo_stats == {"full": 3, "locked": len(js) - 3, "redone": 0}
    assert (5, 5, 2) in seen and (6, 5, 2) in seen                               # clipped at the top: ratios 5, 6
    assert (12, 0, 2) in seen and (13, 0, 2) in seen                             # and at the bottom: ratios 0, 1
    assert [w["matches"][0]["tempo_num"] for w in got] == [NUMS[j] for j in js]


@pytest.mark.parametrize("what", ["empty", "track", "jump"])
def test_what_unlocks_a_channel(what):
    """Window 4 of a channel locked at (1, 3) finds nothing / another track inside the lock's ratios / the same track two
    grid steps away: it is identified twice, reported once with the whole-grid result, and the run starts again."""
    hit = {"empty": None, "track": (5, 3), "jump": (1, 5)}[what]
    script = [[(1, 3)] * 4 + [hit] + [(1, 5)] * 5]
    fake, mon = _monitor(script)
    got = _feed(mon, ROWS_FOR(10), 10)[0]
    seen = _flat(fake.calls)
    assert seen[:6] == [(0, 0, R), (1, 0, R), (2, 0, R), (3, 2, 3), (4, 2, 3), (4, 0, R)]      # window 4: twice
    assert len(got) == 10 and [w["start_s"] for w in got] == [float(i) for i in range(10)]     # each reported once
    assert got[3]["locked"] and not got[4]["locked"]
    if hit is None:
        assert got[4]["matches"] == []
        relock = 8                                                               # windows 5, 6, 7 agree again
    else:
        assert (got[4]["matches"][0]["track"], got[4]["matches"][0]["tempo_num"]) == (hit[0], NUMS[hit[1]])
        relock = 8 if what == "track" else 7                                     # "jump": window 4 starts the new run
    assert seen[6:] == [(w, 0, R) if w < relock else (w, 4, 3) for w in range(5, 10)]
    assert [w["locked"] for w in got[5:]] == [w >= relock for w in range(5, 10)]
    assert mon.tempo_stats == {"full": 3 + 1 + (relock - 5), "locked": 1 + (10 - relock), "redone": 1}


def test_reset_clears_the_lock_and_the_run():
    fake, mon = _monitor([[(1, 3)] * 12])
    _feed(mon, ROWS_FOR(5), 10)
    assert mon._lock[0] == (1, 3) and len(mon._run[0]) == 3
    mon.reset(0)
    assert mon._lock[0] is None and mon._run[0] == []
    fake.calls.clear()
    got = _feed(mon, ROWS_FOR(4), 10)[0]
    assert _flat(fake.calls) == [(0, 0, R), (1, 0, R), (2, 0, R), (3, 2, 3)] and len(got) == 4


def test_two_channels_in_different_states_share_a_launch():
    """Channel 0 locks after three windows; channel 1 finds nothing until window 3.  One window per channel and push:
    every push is one launch for both channels, each item with its own ratio window."""
    script = [[(1, 5)] * 6, [None] * 3 + [(4, 1)] * 3]
    fake, mon = _monitor(script, channels=2)
    per = int(np.ceil(16000 / 1536))
    got = [[], []]
    for lo in range(0, ROWS_FOR(6), per):
        out = mon.push_rows([_rows(0, lo, lo + per), _rows(1, lo, lo + per)])
        assert sum(len(o) for o in out) in (0, 2)
        got[0] += out[0]
        got[1] += out[1]
    assert len(got[0]) == len(got[1]) == 6
    assert fake.calls == [[(0, w, 0, R), (1, w, 0, R)] for w in range(3)] + \
        [[(0, w, 4, 3), (1, w, 0, R)] for w in range(3, 6)]
    assert [w["locked"] for w in got[0]] == [False] * 3 + [True] * 3 and not any(w["locked"] for w in got[1])
    assert mon._lock == [(1, 5), (4, 1)] and all(w["channel"] == c for c in (0, 1) for w in got[c])
    # the next round: channel 1 is locked too, at the bottom of the grid; channel 0 changes track and is redone alone
    script[0].append((3, 5))
    script[1].append((4, 0))
    fake.calls.clear()
    fed = -(-ROWS_FOR(6) // per) * per
    out = mon.push_rows([_rows(0, fed, ROWS_FOR(7)), _rows(1, fed, ROWS_FOR(7))])
    assert fake.calls == [[(0, 6, 4, 3), (1, 6, 0, 3)], [(0, 6, 0, R)]]
    assert (out[0][0]["matches"][0]["track"], out[0][0]["locked"], out[1][0]["locked"]) == (3, False, True)
    assert mon.tempo_stats["redone"] == 1


def test_the_calls_do_not_depend_on_the_chunking():
    """Two channels fed the same number of rows per push, in chunks of 0.5 s, 1 s and 2.5 s of segments: the sequence of
    launches -- which windows, which ratio windows, which redone -- and the windows reported are the same."""
    script = [[(1, 3)] * 4 + [(1, 5)] + [(1, 5)] * 3 + [None] + [(2, 0)] * 5,
              [(4, 6)] * 5 + [(0, 6)] * 4 + [(0, 5), (0, 4), (0, 2), (0, 2), (0, 2)]]
    logs, reported, stats = [], [], []
    for seconds in (0.5, 1.0, 2.5):
        fake, mon = _monitor(script, channels=2)
        got = _feed(mon, ROWS_FOR(14), int(round(seconds * 16000 / 1536)))
        logs.append(fake.calls)
        reported.append(got)
        stats.append(mon.tempo_stats)
    assert logs[0] == logs[1] == logs[2] and reported[0] == reported[1] == reported[2]
    assert stats[0] == stats[1] == stats[2] and stats[0]["redone"] >= 4 and stats[0]["locked"] >= 6
    assert len(reported[0][0]) == len(reported[0][1]) == 14
    assert any(len(call) == 1 for call in logs[0]) and any(len(call) == 2 for call in logs[0])


def test_without_a_lock_one_launch_takes_the_whole_grid_and_no_window_is_marked():
    fake, mon = _monitor([[(1, 3)] * 6], lock=0)
    got = _feed(mon, ROWS_FOR(6), 200)[0]
    assert fake.calls == [[(0, w, 0, R) for w in range(6)]]                     # one launch, no item_ratios
    assert all(list(w) == KEYS for w in got) and mon.tempo_stats == {"full": 6, "locked": 0, "redone": 0}
    assert mon.timeline(0) and all(s["tempo"] == 1.0 for s in mon.timeline(0))


def test_without_tempo_nothing_changes():
    """tempo=None: the hook is called as before (a fake written without item_ratios works), the windows have the
    parent's keys, and the monitor carries no tempo state."""
    fake = Scripted([[(1, 3)] * 6], takes_item_ratios=False)
    mon = monitor.StreamMonitor(fake.lib, 1)
    got = _feed(mon, ROWS_FOR(6), 13)[0]
    assert len(got) == 6 and all(list(w) == KEYS for w in got)
    assert all(list(w["matches"][0]) == ["track", "name", "offset", "offset_s", "score", "votes"] for w in got)
    assert mon.tempo is None and mon.tempo_nums is None and mon.tempo_lock == 0 and not hasattr(mon, "tempo_stats")
    assert [c for call in fake.calls for c in call] == [(0, w) for w in range(6)]
    # and an old-style fake still serves tempo without a lock
    old = Scripted([[(1, 3)] * 3], takes_item_ratios=False)
    assert len(_feed(monitor.StreamMonitor(old.lib, 1, tempo=TEMPO, tempo_step=STEP), ROWS_FOR(3), 50)[0]) == 3


def test_refusals():
    lib = Scripted([[]]).lib
    with pytest.raises(ValueError, match="tempo_lock"):
        monitor.StreamMonitor(lib, 1, tempo_lock=2)                              # a lock without tempo
    with pytest.raises(ValueError, match="tempo_lock"):
        monitor.StreamMonitor(lib, 1, tempo=0.06, tempo_lock=-1)
    with pytest.raises(ValueError, match="tempo"):
        monitor.StreamMonitor(lib, 1, tempo=0.7)
    with pytest.raises(ValueError, match="step"):
        monitor.StreamMonitor(lib, 1, tempo=0.5, tempo_step=1)                   # 257 ratios
    with pytest.raises(NotImplementedError, match="tempo"):
        monitor.StreamMonitor(lib, 1, tempo=0.06, query_stride=2)
    with pytest.raises(NotImplementedError, match=r"StreamMonitor\(tempo"):
        monitor.StreamMonitor(lib.thin(2), 1, tempo=0.06)
    half = FingerprintLibrary.from_half(None, load_config(), torch.zeros((8, 128), dtype=torch.bfloat16), [0, 8],
                                        device="cpu")
    with pytest.raises(NotImplementedError, match="half"):
        monitor.StreamMonitor(half, 1, tempo=0.06)
    with pytest.raises(ValueError, match="ratio_window needs tempo"):
        lib._identify_items(torch.zeros((4, 128)), torch.zeros((4, 1), dtype=torch.int64), [0], [3], 5, None,
                            ratio_window=([0], [1]))


def test_the_op_refuses_bad_ratio_windows_on_the_host():
    rows, q = torch.zeros(8, 128), torch.zeros(30, 128)
    first, ids = torch.tensor([0, 8]), torch.zeros(30, 4, dtype=torch.int64)
    item_row, item_len = torch.tensor([0, 10, 20]), torch.tensor([5, 5, 5], dtype=torch.int32)
    call = lambda lo, cnt, nums=NUMS: ops.identify_tempo_items(rows, first, q, ids, item_row, item_len, nums, lo, cnt)
    for lo, cnt, item in (([0, 5, 0], [7, 3, 1], 1), ([0, 0, -1], [7, 1, 1], 2), ([0, 0, 0], [0, 1, 1], 0),
                          ([0, 0, 7], [7, 7, 1], 2), ([0, 0, 0], [8, 1, 1], 0)):
        with pytest.raises(ValueError, match=f"item {item}'s ratio window"):
            call(lo, cnt)
    with pytest.raises(ValueError, match="one value per item"):
        call([0, 0], [1, 1])
    with pytest.raises(ValueError, match="strictly ascending"):                  # identify_tempo's checks come first
        call([0, 0, 0], [1, 1, 1], [256, 250])
    with pytest.raises(RuntimeError, match="no CPU"):                            # everything on the host passed
        call([0, 2, 4], [7, 3, 3])
    table, n_work, max_cnt = ops.tempo_work_table(7, [0, 2, 6], [2, 3, 1])
    assert table.dtype == np.int32 and (n_work, max_cnt) == (6, 3)
    assert table.tolist() == [0, 0, 0, 1, 1, 2, 1, 3, 1, 4, 2, 6] + [0, 2, 5, 6]


def test_abi_entry_and_workspace():
    from test_abi import _ctype_of, _declared
    from grafp_amd import _lib
    from grafp_amd._lib import lib
    d = _declared()
    ret, args = d["grafp_identify_tempo_items_f32"]
    whole = d["grafp_identify_tempo_f32"][1]
    new = ["const int32_t *work", "int n_work", "const int32_t *item_scan", "int max_cnt"]
    assert ret == "int" and [a for a in args if a not in new] == whole
    assert args[args.index("int n_ratios") + 1:args.index("void *ws")] == new
    res, argtypes = _lib.SIGNATURES["grafp_identify_tempo_items_f32"]
    assert res is ctypes.c_int and [_ctype_of(a) for a in args] == list(argtypes)
    assert d["grafp_identify_tempo_items_workspace"] == ("size_t", ["int n_work", "int top"])
    assert lib.grafp_identify_tempo_items_workspace(123, 5) == 16 * 123 * 5
    assert lib.grafp_identify_tempo_items_workspace(4096 * 64, 64) == 16 * 4096 * 64 * 64
    assert lib.grafp_identify_tempo_items_workspace(0, 5) == 0 and lib.grafp_identify_tempo_items_workspace(-1, 5) == 0
    assert lib.grafp_identify_tempo_items_workspace(4, 65) == 0 and lib.grafp_identify_tempo_items_workspace(4, 0) == 0
    # never dereferenced: every call fails an argument check before anything is launched
    fake = [ctypes.c_void_p(256 * (i + 1)) for i in range(14)]
    nums = (ctypes.c_int32 * 3)(250, 256, 262)

    def call(n_work=8, max_cnt=3, max_len=8, work=fake[12], n_ratios=3):
        return lib.grafp_identify_tempo_items_f32(fake[0], 100, fake[1], 2, fake[2], 1000, fake[3], 4, fake[4], fake[5],
                                                  4, max_len, 5, 0, ctypes.cast(nums, ctypes.c_void_p), n_ratios, work,
                                                  n_work, fake[13], max_cnt, fake[10], fake[6], fake[7], fake[8],
                                                  fake[9], fake[11], None)
    assert call(max_cnt=0) == -1 and b"max_cnt" in lib.grafp_last_error()
    assert call(max_cnt=4) == -1 and b"max_cnt" in lib.grafp_last_error()
    assert call(n_work=3) == -1 and b"n_work" in lib.grafp_last_error()
    assert call(n_work=13) == -1 and b"n_work" in lib.grafp_last_error()
    assert call(max_len=257) == -1 and b"exceed" in lib.grafp_last_error()
    assert call(n_ratios=0) == -1 and b"n_ratios" in lib.grafp_last_error()
    assert call(work=None) == -1 and b"null pointer" in lib.grafp_last_error()


def test_the_kernels_have_no_packed_f32_instructions():
    """The shipped object's own command (make -n), compiled to device assembly: both query-row plans of pass 1 and the
    merge of pass 2, nothing else, none with a packed-f32 instruction or scratch memory."""
    asm = shipped_asm("identify_tempo_items")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert sum("identify_tempo_items_kernel" in k for k in kernels) == 2
    assert sum("identify_tempo_items_merge_kernel" in k for k in kernels) == 1 and len(kernels) == 3
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm) == ["0"] * 3


def test_monitor_takes_a_tempo_on_the_command_line(capsys):
    from grafp_amd import identify
    with pytest.raises(SystemExit) as e:
        identify.main(["monitor", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--tempo" in out and "--tempo-step" in out and "--tempo-lock" in out
