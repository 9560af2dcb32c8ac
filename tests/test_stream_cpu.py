"""The host side of live stream monitoring (grafp_amd/monitor.py) without a GPU: the readiness rules against brute-force
restatements (tests/_stream_ref.py), the frame / segment counts, the carry, the window schedule against
library.window_items, and the refusals.  The two launches of the front end are replaced by _stream_ref.FakeFrontEnd,
which checks every sample a due frame reads."""
import numpy as np
import pytest
import torch

from _stream_ref import FakeFrontEnd, cycle_chunks, random_chunks, read_positions
from grafp_amd import monitor, ops
from grafp_amd.library import FingerprintLibrary, n_segments, segment_step, window_items
from grafp_amd.util import load_config

N_FFT = 1024
LENGTHS = (0, 300, 512, 513, 1023, 1024, 16383, 16384, 16385, 40000)


def _cfg(hop=512):
    cfg = load_config()
    cfg["hop_len"] = hop
    return cfg


def _cpu_library(cfg):
    """A library without rows on the CPU: the monitor's tables and schedule work, nothing is searched or identified."""
    lib = FingerprintLibrary(None, cfg, None, None, device="cpu")
    lib._embed = lambda segs: torch.zeros((segs.shape[0], 128))
    return lib


@pytest.mark.parametrize("hop", [512, 256, 160])
def test_frame_ready_is_the_brute_force_read_set(hop):
    for f in range(0, 14):
        reads = read_positions(f, N_FFT, hop)                        # an open stream: reflected at the start only
        for seen in list(range(0, 1100, 37)) + [int(reads.max()) + d for d in (-1, 0, 1, 2)]:
            assert monitor.frame_ready(f, seen, N_FFT, hop) == bool(reads.max() < seen), (f, seen)
    for seen in list(range(0, 3000, 61)) + [512, 513, 1023, 1024, 1025, 1535, 1536, 1537]:
        ready = [bool(read_positions(f, N_FFT, hop).max() < seen) for f in range(seen // hop + 3)]
        count = 0
        while count < len(ready) and ready[count]:
            count += 1
        assert all(not r for r in ready[count:])                     # once a frame is ready all earlier ones are
        assert monitor.frames_ready(seen, False, N_FFT, hop) == count - (count & 1), seen


@pytest.mark.parametrize("hop", [512, 256])
def test_counts_after_end(hop, monkeypatch):
    """An ended stream has the frames of ops.logmel (1 + T // hop; a waveform of T <= n_fft/2 samples, which ops.logmel
    refuses, has none) and the segments library.n_segments counts -- by the rules and through the front end's state."""
    cfg = _cfg(hop)
    step, n_frames = segment_step(cfg), cfg["n_frames"]
    rng = np.random.RandomState(5)
    whole = [rng.randn(T).astype(np.float32) for T in LENGTHS]
    for T in LENGTHS:
        frames = monitor.frames_ready(T, True, N_FFT, hop)
        assert frames == (1 + T // hop if T > N_FFT // 2 else 0), T
        assert monitor.segments_ready(frames, n_frames, step) == n_segments(T, cfg), T
    fake = FakeFrontEnd(whole, N_FFT, hop).install(monkeypatch)
    front = monitor.StreamFrontEnd(cfg, len(LENGTHS), "cpu", max_chunk_s=0.256)
    assert front.R == 64
    plans = [cycle_chunks(T, i) for i, T in enumerate(LENGTHS)]
    pos = [0] * len(LENGTHS)
    for r in range(max(len(p) for p in plans)):
        chunks = []
        for c, p in enumerate(plans):
            n = p[r] if r < len(p) else 0
            chunks.append(torch.from_numpy(whole[c][pos[c]:pos[c] + n]) if n else None)
            pos[c] += n
        segs, counts = front.push(chunks)
        assert segs.shape[0] == counts.sum()
        for c in range(len(LENGTHS)):                                # open: whole pairs of ready frames, no more
            assert front.frames[c] == monitor.frames_ready(pos[c], False, N_FFT, hop)
    front.end(range(len(LENGTHS)))
    for c, T in enumerate(LENGTHS):
        assert front.seen[c] == T
        assert front.frames[c] == (1 + T // hop if T > N_FFT // 2 else 0), T
        assert front.segs[c] == n_segments(T, cfg), T
        got = [f for a, b in fake.frame_ranges[c] for f in range(a, b)]
        assert got == list(range(int(front.frames[c]))), T          # every frame once, in order
        got = [s for a, b in fake.seg_ranges[c] for s in range(a, b)]
        assert got == list(range(int(front.segs[c]))), T


@pytest.mark.parametrize("seed", range(6))
def test_the_carry_never_drops_a_sample_a_later_frame_reads(seed, monkeypatch):
    """Random chunkings (zeros and single samples among them, chunks longer than max_chunk_s fed in pieces): FakeFrontEnd
    asserts that every sample of every due frame is in the buffer and is the stream's sample at that position; the
    carry stays short."""
    hop = (512, 256, 160)[seed % 3]
    cfg = _cfg(hop)
    rng = np.random.RandomState(100 + seed)
    lengths = [int(rng.randint(600, 30000)) for _ in range(3)] + [int(rng.randint(0, 600))]
    whole = [rng.randn(T).astype(np.float32) for T in lengths]
    fake = FakeFrontEnd(whole, N_FFT, hop).install(monkeypatch)
    front = monitor.StreamFrontEnd(cfg, 4, "cpu", max_chunk_s=0.3)
    plans = [random_chunks(T, 1000 * seed + c) for c, T in enumerate(lengths)]
    pos = [0] * 4
    for r in range(max(len(p) for p in plans)):
        chunks = []
        for c, p in enumerate(plans):
            n = p[r] if r < len(p) else 0
            chunks.append(torch.from_numpy(whole[c][pos[c]:pos[c] + n]) if n else None)
            pos[c] += n
        front.push(chunks)
        for c in range(4):
            k = front._carry[c]
            assert front.base[c] + (0 if k is None else k.numel()) == front.seen[c] == pos[c]
            assert (0 if k is None else k.numel()) <= N_FFT + 2 * hop            # left edge of the next pair + a partner
            assert front.base[c] == monitor.keep_from(front.frames[c], pos[c], N_FFT, hop)
    front.end([0, 1, 2, 3])
    for c, T in enumerate(lengths):
        assert front.frames[c] == (1 + T // hop if T > N_FFT // 2 else 0)
        assert [f for a, b in fake.frame_ranges[c] for f in range(a, b)] == list(range(int(front.frames[c])))
    with pytest.raises(ValueError, match="has ended"):
        front.push([torch.zeros(5), None, None, None])


def _check_prefix(cfg, lengths, plans, window_s, hop_s, monkeypatch):
    rng = np.random.RandomState(3)
    C = len(lengths)
    whole = [rng.randn(T).astype(np.float32) for T in lengths]
    FakeFrontEnd(whole, N_FFT, cfg["hop_len"]).install(monkeypatch)
    mon = monitor.StreamMonitor(_cpu_library(cfg), C, window_s=window_s, hop_s=hop_s, max_chunk_s=0.5)
    final = [window_items(n_segments(T, cfg), T, cfg, window_s, hop_s) for T in lengths]
    seg_s = segment_step(cfg) * cfg["hop_len"] / cfg["fs"]
    pos, emitted = [0] * C, [[] for _ in range(C)]

    def listed(c):
        """Windows window_items lists with their full length for what channel c has seen so far."""
        S = monitor.segments_ready(monitor.frames_ready(pos[c], False, N_FFT, cfg["hop_len"]), cfg["n_frames"],
                                   segment_step(cfg))
        _, _, lens = window_items(S, pos[c], cfg, window_s, hop_s)
        n = 0
        while n < len(lens) and lens[n] == mon.per_window:
            n += 1
        return n

    for r in range(max(len(p) for p in plans)):
        chunks = []
        for c, p in enumerate(plans):
            n = p[r] if r < len(p) else 0
            chunks.append(whole[c][pos[c]:pos[c] + n] if n else (None if r % 2 else np.zeros(0, np.float32)))
            pos[c] += n
        out = mon.push(chunks)
        for c in range(C):
            emitted[c] += out[c]
            assert len(emitted[c]) == listed(c), (c, r)             # by the FIRST push after which it is listed
    for c in range(C):
        emitted[c] += mon.end(c)
        starts, rows, lens = final[c]
        assert len(emitted[c]) == len(starts)                        # all of them, each once
        for w, win in enumerate(emitted[c]):
            assert win == {"start_s": float(starts[w]), "end_s": float(starts[w]) + window_s,
                           "segment_start_s": int(rows[w]) * seg_s, "matches": [], "channel": c}
        assert mon.windows(c) == emitted[c] and mon.end(c) == []
        assert mon.timeline(c) == []


@pytest.mark.parametrize("seed", range(4))
def test_windows_are_a_prefix_of_window_items_over_random_chunkings(seed, monkeypatch):
    cfg = _cfg()
    rng = np.random.RandomState(40 + seed)
    lengths = [int(rng.randint(50000, 120000)), int(rng.randint(16000, 50000)), 48000, int(rng.randint(0, 16000))]
    plans = [random_chunks(T, 7 * seed + c, big=12000) for c, T in enumerate(lengths)]
    window_s, hop_s = ((3.0, 1.0), (1.5, 0.5), (3.0, 0.7), (2.0, 2.5))[seed]
    _check_prefix(cfg, lengths, plans, window_s, hop_s, monkeypatch)


def test_a_window_waits_for_its_samples_not_only_for_its_segments(monkeypatch):
    """Window 12 of the default schedule starts at sample 192 000 = segment 125 exactly.  Its 21 segments (the last one
    ends with frame 466, whose partner 467 needs 239 616 samples) exist 384 samples before identify_windows counts the
    window (240 000 samples = 3 s + 12 s): it is reported by the push that brings sample 240 000, not before.  Window 0
    is the other way round: a recording of at most 3 s is one window, so it is reported as soon as its segments exist."""
    cfg = _cfg()
    x = np.zeros(241000, np.float32)
    FakeFrontEnd([x], N_FFT, 512).install(monkeypatch)
    mon = monitor.StreamMonitor(_cpu_library(cfg), 1, max_chunk_s=1.0)
    assert mon.per_window == 21
    assert mon.push([x[:47103]]) == [[]]
    assert [w["start_s"] for w in mon.push([x[47103:47104]])[0]] == [0.0]
    assert [w["start_s"] for w in mon.push([x[47104:239616]])[0]] == [float(w) for w in range(1, 12)]
    assert int(mon._n_rows[0]) == 125 + 21                            # the segments of window 12 are there
    assert mon.push([x[239616:239999]]) == [[]]
    got = mon.push([x[239999:240000]])[0]
    assert [w["start_s"] for w in got] == [12.0] and got[0]["segment_start_s"] == 125 * mon.library.segment_s
    assert mon.push([None]) == [[]]


def test_push_rows_schedules_like_push(monkeypatch):
    """Rows in uneven slices: the windows are the prefix property's, and end() takes the final sample count."""
    cfg = _cfg()
    T = 100000
    S = n_segments(T, cfg)
    mon = monitor.StreamMonitor(_cpu_library(cfg), 2)
    starts, rows, lens = window_items(S, T, cfg, 3.0, 1.0)
    got, fed = [], 0
    assert S == 55
    for n in (1, 0, 20, 7, 12, S - 40):
        out = mon.push_rows([torch.zeros((n, 128)) if n else None, None])
        fed += n
        got += out[0]
        _, _, now = window_items(fed, monitor.samples_lower_bound(fed, cfg), cfg, 3.0, 1.0)
        assert len(got) == int((np.cumprod(now == 21)).sum()) and out[1] == []
    with pytest.raises(ValueError, match="push_rows"):
        mon.push([np.zeros(10, np.float32), None])
    with pytest.raises(ValueError, match="n_samples"):
        mon.end(0)
    with pytest.raises(ValueError, match="segments"):
        mon.end(0, n_samples=T + 5000)
    got += mon.end(0, n_samples=T)
    assert [w["start_s"] for w in got] == [float(s) for s in starts]
    assert [w["segment_start_s"] for w in got] == [int(r) * mon.library.segment_s for r in rows]
    with pytest.raises(ValueError, match="has ended"):
        mon.push_rows([torch.zeros((1, 128)), None])
    mon.reset(0)
    assert mon.windows(0) == [] and mon.push_rows([torch.zeros((3, 128)), None]) == [[], []]


def test_refusals():
    cfg = _cfg()
    lib = _cpu_library(cfg)
    mon = monitor.StreamMonitor(lib, 3)
    with pytest.raises(ValueError, match="3 channels"):
        mon.push([np.zeros(4, np.float32)] * 2)
    with pytest.raises(ValueError, match="3 channels"):
        mon.push_rows([None] * 4)
    with pytest.raises(ValueError, match="1-D"):
        mon.push([np.zeros((2, 4), np.float32), None, None])
    assert mon.push([None, np.zeros(0, np.float32), None]) == [[], [], []]
    bad = dict(cfg, n_fft=512, win_len=512)
    with pytest.raises(ValueError, match="n_fft == 1024"):
        monitor.StreamMonitor(_cpu_library(bad), 2)
    with pytest.raises(ValueError, match="n_fft == 1024"):
        monitor.StreamMonitor(_cpu_library(dict(cfg, n_mels=128)), 2)
    with pytest.raises(ValueError, match="exceeds"):                  # 30 s: 303 segments per window, identify takes 256
        monitor.StreamMonitor(lib, 2, window_s=30.0)
    with pytest.raises(ValueError, match="exceeds"):                  # 21 * 400 hits > 8192 keys
        monitor.StreamMonitor(lib, 2, k_probe=400)
    with pytest.raises(ValueError, match="shorter than one segment"):
        monitor.StreamMonitor(lib, 2, window_s=0.5)
    with pytest.raises(ValueError, match="at least 1"):
        monitor.StreamMonitor(lib, 0)


def test_the_ops_refuse_cpu_tensors_and_bad_tables():
    ring = torch.zeros((1, 64, 64))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.stream_logmel(torch.zeros(2048), [0], [2048], [0], [2048], [False], [0], [2], ring)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.stream_segments(ring, [0], [1], 32, 3)
    plan = lambda **kw: ops.stream_logmel_plan(**{**dict(
        n_channels=1, ring_len=64, bank_len=4096, starts=[0], lengths=[2048], base=[0], seen=[2048], ended=[False],
        frame_lo=[0], frame_hi=[2], n_fft=1024, hop=512), **kw})
    assert plan()[5].tolist() == [0, 1]
    assert plan(frame_hi=[0]) is None
    for kw in (dict(frame_lo=[1], frame_hi=[3]),                      # off the offline kernel's pair grid
               dict(frame_hi=[3]),                                    # an open stream and an odd count
               dict(frame_hi=[6]),                                    # frame 5 reads up to sample 3071
               dict(lengths=[2049]),                                  # the buffer does not end at `seen`
               dict(base=[100], lengths=[1948]),                      # frame 0 reflects at the stream's start
               dict(bank_len=2000),
               dict(frame_hi=[66], seen=[40000], lengths=[40000], bank_len=40000),   # more frames than the ring holds
               dict(ended=[True], frame_hi=[6])):                     # an ended stream of 2048 samples has 5 frames
        with pytest.raises(ValueError):
            plan(**kw)
    assert plan(ended=[True], frame_hi=[5])[5].tolist() == [0, 1]


def test_command_line_parses_monitor(capsys):
    from grafp_amd import identify
    with pytest.raises(SystemExit) as e:
        identify.main(["monitor", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--chunk-s" in out and "LIBDIR" in out and "--window" in out
    with pytest.raises(SystemExit) as e:
        identify.main(["monitor", "--ckp", "m.pth", "libdir"])       # the files are required
    assert e.value.code == 2
