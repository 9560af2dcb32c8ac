"""Live stream monitoring on the MI355X: the two launches of csrc/stream_frontend.hip against ops.logmel /
FingerprintLibrary.segments on the concatenated stream, bit for bit, after every push; the window schedule of
StreamMonitor.push_rows against FingerprintLibrary.identify_windows in every field on a flat, a thinned and a compact
library; push() on waveforms end to end."""
import numpy as np
import pytest
import torch

from _retrieval_case import synth_tracks
from _stream_ref import CHUNK_CYCLE, cycle_chunks
from grafp_amd import ops
from grafp_amd.library import FingerprintLibrary
from grafp_amd.monitor import StreamFrontEnd, StreamMonitor
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
LENGTHS = (40000, 17000, 600, 300)
MAX_CHUNK_S = 4096 / 16000            # the longest chunk of the cycle: R = 64, the 79 frames of channel 0 wrap the ring


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def streams(dev):
    """Four channels of seeded noise and, computed once, what the offline path makes of each whole stream."""
    cfg = load_config()
    g = torch.Generator().manual_seed(77)
    whole = [(0.1 * torch.randn(T, generator=g)).to(dev) for T in LENGTHS]
    lib = FingerprintLibrary(None, cfg, None, None, device=dev)
    spec = [ops.logmel(x, cfg["fs"], cfg["n_fft"], cfg["win_len"], cfg["hop_len"], cfg["n_mels"])
            if x.numel() > cfg["n_fft"] // 2 else torch.empty((cfg["n_mels"], 0), device=dev) for x in whole]
    segs = [lib.segments(x) if x.numel() > cfg["n_fft"] // 2 else lib.segments(x[:0]) for x in whole]
    assert [s.shape[1] for s in spec] == [79, 34, 2, 0] and [s.shape[0] for s in segs] == [16, 1, 0, 0]
    return cfg, whole, spec, segs


def _frames(front, c, n_mels, dev):
    log = front.frames_log[c]
    return torch.cat(log, dim=1) if log else torch.empty((n_mels, 0), device=dev)


def test_frames_and_segments_are_the_offline_bits_after_every_push(streams, dev):
    cfg, whole, spec, segs = streams
    C = len(LENGTHS)
    front = StreamFrontEnd(cfg, C, dev, max_chunk_s=MAX_CHUNK_S, record_frames=True)
    assert front.R == 64
    plans = [cycle_chunks(T, 2 * c) for c, T in enumerate(LENGTHS)]   # out of phase per channel
    assert set(CHUNK_CYCLE) <= set(plans[0])
    pos, got_segs = [0] * C, [[] for _ in range(C)]
    for r in range(max(len(p) for p in plans)):
        chunks = []
        for c, p in enumerate(plans):
            n = p[r] if r < len(p) else 0
            chunks.append(whole[c][pos[c]:pos[c] + n] if n else None)
            pos[c] += n
        new, counts = front.push(chunks)
        assert new.shape[0] == counts.sum()
        for c, part in enumerate(torch.split(new, counts.tolist())):
            got_segs[c].append(part)
            F, S = int(front.frames[c]), int(front.segs[c])
            assert F % 2 == 0 and F <= spec[c].shape[1]
            assert torch.equal(_frames(front, c, cfg["n_mels"], dev), spec[c][:, :F]), (r, c, F)
            assert torch.equal(torch.cat(got_segs[c]), segs[c][:S]), (r, c, S)
    assert [int(f) for f in front.frames] == [78, 32, 0, 0]           # what an open stream can know
    new, counts = front.end(range(C))
    assert counts.tolist() == [0, 0, 0, 0]                            # (the last frames complete no further segment here)
    for c, part in enumerate(torch.split(new, counts.tolist())):
        got_segs[c].append(part)
        assert torch.equal(_frames(front, c, cfg["n_mels"], dev), spec[c]), c
        assert torch.equal(torch.cat(got_segs[c]), segs[c]), c
    assert [int(f) for f in front.frames] == [79, 34, 2, 0] and [int(s) for s in front.segs] == [16, 1, 0, 0]


def test_one_push_and_end_give_the_same_bits(streams, dev):
    cfg, whole, spec, segs = streams
    C = len(LENGTHS)
    front = StreamFrontEnd(cfg, C, dev, max_chunk_s=MAX_CHUNK_S, record_frames=True)
    a, na = front.push(list(whole))                                   # fed in pieces of 4096 samples: ten front-end steps
    b, nb = front.end(range(C))
    for c in range(C):
        assert torch.equal(_frames(front, c, cfg["n_mels"], dev), spec[c]), c
        got = torch.cat([torch.split(a, na.tolist())[c], torch.split(b, nb.tolist())[c]])
        assert torch.equal(got, segs[c]), c
    assert front.launches <= 2 * 11                                   # two per step, however many channels


@pytest.fixture(scope="module")
def case(dev):
    """A flat f32 library of 6 short tracks (untrained model) and a 12 s stream made of excerpts of two of them, cut from
    and placed at multiples of the segment hop."""
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    tracks = synth_tracks(6, 84 * SEG_HOP / 16000, 4242, dev)        # 8.06 s each
    lib = FingerprintLibrary.build(model, list(tracks), cfg, names=[f"song{i}" for i in range(6)], precision="f32",
                                   max_segments=200)
    cuts = [(1, 5, 63), (4, 12, 62)]                                  # (track, first segment hop, segment hops)
    stream = torch.cat([tracks[t, j * SEG_HOP:(j + n) * SEG_HOP] for t, j, n in cuts]).contiguous()
    assert stream.numel() == 12 * 16000
    return cfg, lib, stream, cuts


@pytest.mark.parametrize("form", ["flat", "thin", "compact"])
def test_push_rows_reports_the_windows_of_identify_windows(case, dev, form):
    """Search ids are exact and identify's scores depend only on the rows, so the windows must agree in every field,
    scores bit for bit, however the rows are sliced."""
    cfg, flat, stream, _ = case
    lib = {"flat": lambda: flat, "thin": lambda: flat.thin(2),
           "compact": lambda: flat.compress(nlist=4, pq_m=16)}[form]()
    want = lib.identify_windows(stream)
    rows = lib._embed(lib.segments(stream))
    assert rows.shape[0] == 115 and len(want) == 10 and all(w["matches"] for w in want)
    mon = StreamMonitor(lib, 2)
    got, lo = [], 0
    for n in (1, 20, 0, 33, 7, 2, 40, 12):                            # uneven slices; channel 0 stays silent
        out = mon.push_rows([None, rows[lo:lo + n] if n else None])
        assert out[0] == []
        got += out[1]
        lo += n
    assert lo == 115 and 0 < len(got) < len(want)
    got += mon.end(1, n_samples=stream.numel())
    assert [{k: v for k, v in w.items() if k != "channel"} for w in got] == want
    assert all(w["channel"] == 1 for w in got)
    assert mon.timeline(1) == lib.timeline(want)
    assert mon.end(0) == [{"start_s": 0.0, "end_s": 3.0, "segment_start_s": 0.0, "matches": [], "channel": 0}]


def test_push_of_waveforms_end_to_end(case, dev):
    """1 s chunks on channel 1 of three (channel 0 gets the same stream in one push, channel 2 nothing).  Every window
    inside one excerpt names its track with offset_s within one segment hop of the truth (the bounds of
    test_clean_grid_crops_are_identified: the true alignment pairs exact rows); the timeline lists the two tracks in
    order (see the note on the windows across the cut below).  Scores are not compared with the offline path: the segments reach the model in other batches."""
    cfg, lib, stream, cuts = case
    mon = StreamMonitor(lib, 3, max_chunk_s=1.0)
    assert mon.push([None, None, None]) == [[], [], []] and mon.front.launches == 0
    assert mon.push([stream[:0], None, np.zeros(0, np.float32)]) == [[], [], []] and mon.front.launches == 0
    wins = [[], [], []]
    for s in range(12):
        before = mon.front.launches
        out = mon.push([stream if s == 0 else None, stream[s * 16000:(s + 1) * 16000], None])
        assert mon.front.launches - before <= (2 if s else 2 * 12)   # two launches for all channels (12 pieces at s = 0)
        for c in range(3):
            wins[c] += out[c]
    assert len(wins[0]) == len(wins[1]) == 10 and wins[2] == []      # 12 s seen: window_items lists all ten in full
    for c, out in enumerate(mon.end([0, 1, 2])):
        wins[c] += out
    offline = lib.identify_windows(stream)
    assert len(offline) == 10
    seg_s = SEG_HOP / 16000
    for c in (0, 1):
        assert [(w["start_s"], w["end_s"], w["segment_start_s"], w["channel"]) for w in wins[c]] == \
            [(w["start_s"], w["end_s"], w["segment_start_s"], c) for w in offline]
        inside = 0
        for w in wins[c]:
            j0 = int(round(w["segment_start_s"] / seg_s))
            # the samples its 21 segments read (the first frame of the stream reflects at sample 0 instead)
            first, last = max(0, j0 * SEG_HOP - 512), (j0 + 20) * SEG_HOP + 31 * 512 + 512
            pos = 0
            for t, j, n in cuts:
                if pos <= first and last <= pos + n * SEG_HOP:
                    inside += 1
                    m = w["matches"][0]
                    truth = (j0 - pos // SEG_HOP + j) * seg_s
                    assert m["track"] == t and m["name"] == f"song{t}", (c, w["start_s"], w["matches"][:2])
                    assert abs(m["offset_s"] - truth) <= seg_s + 1e-9, (c, w["start_s"], m, truth)
                pos += n * SEG_HOP
        assert inside == 7                                            # windows 0-3 and 7-9
        # The timeline lists the two tracks in order: windows 0-3 lie inside the first excerpt and merge into one span
        # from 0 s, windows 7-9 inside the second and merge into one span up to 12 s.  The windows at 4, 5 and 6 s lie
        # across the cut and have no true alignment; whatever they name sits between the two.  (With this untrained
        # model all cosines are above 0.9999, and library.timeline(identify_windows(stream)) itself puts a span of a
        # third track there: the window at 4 s scores song2 0.9999963 against song1 0.9999960.  Measured on MI355X.)
        spans = mon.timeline(c)
        a, b = spans[0], spans[-1]
        assert a["track"] == cuts[0][0] and a["start_s"] == 0.0 and a["end_s"] >= 6.0, spans
        assert b["track"] == cuts[1][0] and b["start_s"] <= 7.0 and b["end_s"] == 12.0, spans
        assert abs(a["track_offset_s"] - cuts[0][1] * seg_s) <= seg_s + 1e-9
        assert all(4.0 <= s["start_s"] and s["end_s"] <= 9.0 for s in spans[1:-1]), spans
    assert wins[2] == [{"start_s": 0.0, "end_s": 3.0, "segment_start_s": 0.0, "matches": [], "channel": 2}]
    # a new stream on an ended channel
    with pytest.raises(ValueError, match="has ended"):
        mon.push([stream[:100], None, None])
    mon.reset(0)
    again = mon.push([stream[:5 * 16000], None, None])[0] + mon.end(0)
    assert [w["start_s"] for w in again] == [0.0, 1.0, 2.0] and mon.windows(0) == again


def test_command_line_monitor_follows_files_as_channels(case, dev, tmp_path, capsys):
    """python -m grafp_amd.identify monitor: one JSON line per window as it becomes due, then the timelines."""
    import json

    from grafp_amd import identify
    cfg, lib, stream, cuts = case
    torch.save({"state_dict": lib.model.state_dict()}, str(tmp_path / "model.pth"))
    lib.save(str(tmp_path / "lib"))
    files = [str(tmp_path / "feed0.npy"), str(tmp_path / "feed1.npy")]
    np.save(files[0], stream.cpu().numpy())
    np.save(files[1], stream[:40000].cpu().numpy())
    capsys.readouterr()
    assert identify.main(["monitor", "--ckp", str(tmp_path / "model.pth"), str(tmp_path / "lib"), *files,
                          "--chunk-s", "1.0"]) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    wins = [ln for ln in lines if "span" not in ln]
    spans = [ln for ln in lines if "span" in ln]
    assert [w["start_s"] for w in wins if w["channel"] == 0] == [float(s) for s in range(10)]
    assert [w["start_s"] for w in wins if w["channel"] == 1] == [0.0]             # 2.5 s: one short window, at the end
    assert all(w["file"] == files[w["channel"]] and w["matches"] for w in wins)
    own = [s["span"] for s in spans if s["channel"] == 0]
    assert own[0]["track"] == cuts[0][0] and own[0]["start_s"] == 0.0 and own[-1]["track"] == cuts[1][0]
    assert own[-1]["end_s"] == 12.0 and any(s["channel"] == 1 for s in spans)
    assert lines.index(wins[-1]) < lines.index(spans[0])
