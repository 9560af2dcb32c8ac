"""Monitor live multi-channel audio against a fingerprint library.

A StreamMonitor listens to `channels` feeds at once (radio stations, venue microphones) and says what is playing on
each, a window or so behind real time.  Audio arrives through push(): one ragged chunk per channel.  Only the NEW
samples are turned into log-mel frames and segments -- by the two launches of csrc/stream_frontend.hip, whatever the
number of channels -- then all new segments go through one model call and one search, and every window that became due
on any channel through one identify launch.  Nothing a channel already reported is computed again.  With tempo= the
channels may play faster or slower than the catalogue, and with tempo_lock a channel whose speed has shown itself is
searched over three ratios of the grid only (ops.identify_tempo_items; the rule is stated at StreamMonitor).

The contract: for every channel, after any sequence of pushes and end(), the frames and
segments produced so far are the first that many of ops.logmel / FingerprintLibrary.segments on the concatenation of
that channel's chunks, bit for bit, and the windows reported so far are a prefix of what
FingerprintLibrary.identify_windows lists for the finished stream, each reported once.

The rules that make this work are the pure host functions below (tests/test_stream_cpu.py checks them without a GPU):

  frame_ready     while a stream is open, frame f may be computed once every sample the offline kernel reads for it has
                  arrived: max(f hop + n_fft/2 - 1, n_fft/2 - f hop) < seen (the reflection at the stream's START is
                  part of the frame; a reflection at its end never is: the end is not known yet);
  frames_ready    frames are emitted in whole pairs (2p, 2p + 1) while the stream is open -- the kernel carries frame 2p
                  in the real and 2p + 1 in the imaginary part of one transform, so a frame's bits depend on its partner
                  and the pairs must sit on the offline kernel's grid.  A stream that has ended emits all its
                  1 + seen // hop frames, the last ones with the end reflection of torch.stft(center=True), the very last
                  one unpaired if their number is odd -- as ops.logmel does it.  A stream that ends with
                  seen <= n_fft/2 emits nothing (ops.logmel refuses such a waveform);
  segments_ready  segment s is ready when its last frame is emitted;
  keep_from       the first sample the host still needs: min(F hop - n_fft/2, seen - n_fft/2 - 1), clamped at 0, with F
                  the next frame -- the left edge of frame F, or the oldest sample the end reflection would read if the
                  stream ended now;
  ring_length     the spectrogram ring holds R >= n_frames + (the frames one step can add) frames, R a power of two.
"""
import numpy as np
import torch

from . import ops
from .library import kept_items, n_segments, segment_step, tempo_ratios, track_table, window_items


# ---- readiness rules: pure host functions ------------------------------------------------------------------------------
def frame_ready(f, seen, n_fft, hop):
    """Whether frame f of an OPEN stream of `seen` samples can be computed: every position the offline kernel reads for
    it (f * hop + t - n_fft/2 for t in [0, n_fft), reflected at 0) lies below `seen`."""
    half = int(n_fft) // 2
    return max(f * hop + half - 1, half - f * hop) < seen


def frames_ready(seen, ended, n_fft, hop):
    """Frames emitted of a stream of `seen` samples: open, the largest even count whose frames are all ready; ended,
    all 1 + seen // hop of them (none if seen <= n_fft/2)."""
    seen, half, hop = int(seen), int(n_fft) // 2, int(hop)
    if seen <= half:
        return 0
    if ended:
        return 1 + seen // hop
    return ((seen - half) // hop + 1) & ~1


def segments_ready(frames, n_frames, step):
    """Segments whose last frame is among the first `frames` frames."""
    return 0 if frames < n_frames else (int(frames) - int(n_frames)) // int(step) + 1


def keep_from(next_frame, seen, n_fft, hop):
    """The first sample of an open stream that a later frame may still read (everything before it can be dropped)."""
    half = int(n_fft) // 2
    return max(0, min(int(next_frame) * int(hop) - half, int(seen) - half - 1))


def frames_per_step(max_chunk, n_fft, hop):
    """The most frames one front-end step adds: a chunk of max_chunk samples (ceil(max_chunk / hop) more ready frames,
    one more when the even count catches up), or an end (the frames that waited for their right edge, ceil(n_fft/2 / hop)
    of them, the one that waited for a partner and the unpaired last)."""
    half = int(n_fft) // 2
    return max(-(-int(max_chunk) // hop), -(-half // hop)) + 2


def ring_length(max_chunk, n_fft, hop, n_frames):
    """R: the smallest power of two >= n_frames + frames_per_step.  The oldest frame a new segment reads is less than
    n_frames behind the first new frame, so a step never overwrites a frame its own segments read."""
    need, R = int(n_frames) + frames_per_step(max_chunk, n_fft, hop), 2
    while R < need:
        R *= 2
    return R


def samples_lower_bound(n_seg, settings):
    """The fewest samples a stream (open or ended) has when n_seg of its segments exist: the last segment's last frame
    f exists only if 1 + T // hop > f."""
    if n_seg <= 0:
        return 0
    last = (int(n_seg) - 1) * segment_step(settings) + int(settings["n_frames"]) - 1
    return last * int(settings["hop_len"])


def _check_settings(settings):
    if int(settings["n_fft"]) != 1024 or not 1 <= int(settings["n_mels"]) <= 64:
        raise ValueError(f"the stream front end supports only n_fft == 1024 and n_mels <= 64 (the model's configuration), "
                         f"not n_fft={settings['n_fft']}, n_mels={settings['n_mels']}")
    if segment_step(settings) < 1:
        raise ValueError("the stream front end needs a segment step of at least one frame")


class StreamFrontEnd:
    """The per-channel state of the stream front end and its two launches: chunks in, new segments out.

    Per channel it keeps the samples seen, the frames and segments emitted, the carried samples (a view of the last
    step's bank) with the stream position of the first of them, and one row of the (channels, n_mels, R) spectrogram
    ring.  Everything runs on the current stream.  record_frames=True also keeps every emitted frame (per channel, a list
    of (n_mels, new frames) copies): the seam tests/test_gpu_stream.py compares against ops.logmel."""

    def __init__(self, settings, channels, device, max_chunk_s=1.0, record_frames=False):
        _check_settings(settings)
        if int(channels) < 1:
            raise ValueError(f"channels={channels} must be at least 1")
        self.settings, self.channels, self.device = dict(settings), int(channels), torch.device(device)
        c = self.settings
        self.step = segment_step(c)
        self.max_chunk = int(float(max_chunk_s) * c["fs"])
        if self.max_chunk < 1:
            raise ValueError(f"max_chunk_s={max_chunk_s} is less than one sample")
        self.R = ring_length(self.max_chunk, c["n_fft"], c["hop_len"], c["n_frames"])
        C = self.channels
        self.seen, self.frames, self.segs, self.base = (np.zeros(C, np.int64) for _ in range(4))
        self.ended = np.zeros(C, bool)
        self._carry = [None] * C
        self._ring = None                       # made on the first step: a monitor on a CPU device holds tables only
        self.frames_log = [[] for _ in range(C)] if record_frames else None
        self.launches = 0                       # front-end launches so far (stream_logmel + stream_segments)

    def reset(self, channel):
        c = int(channel)
        self.seen[c] = self.frames[c] = self.segs[c] = self.base[c] = 0
        self.ended[c] = False
        self._carry[c] = None
        if self.frames_log is not None:
            self.frames_log[c] = []

    def _empty(self):
        c = self.settings
        return torch.empty((0, c["n_mels"], c["n_frames"]), dtype=torch.float32, device=self.device)

    def push(self, chunks):
        """chunks: per channel a 1-D f32 device tensor at settings['fs'], or None.  A chunk longer than max_chunk_s is
        fed in pieces (the ring is sized for one piece).  -> (new segments (n, n_mels, n_frames), per-channel counts),
        the segments packed channel by channel."""
        lens = np.array([0 if w is None else int(w.numel()) for w in chunks], np.int64)
        if (lens > 0)[self.ended].any():
            raise ValueError("push: a channel that has ended takes no more audio; reset() starts a new stream on it")
        C, mc = self.channels, self.max_chunk
        rounds = int(-(-int(lens.max(initial=0)) // mc))
        if rounds <= 1:
            return self._step(chunks, lens, np.zeros(C, bool))
        per_round = []
        for r in range(rounds):
            pieces = [None if lens[c] <= r * mc else chunks[c][r * mc:(r + 1) * mc] for c in range(C)]
            per_round.append(self._step(pieces, np.clip(lens - r * mc, 0, mc), np.zeros(C, bool)))
        return self._merge(per_round)

    def end(self, channels):
        """The listed channels have ended: the frames and segments that waited for more audio are flushed."""
        ending = np.zeros(self.channels, bool)
        ending[np.asarray(list(channels), np.int64)] = True
        ending &= ~self.ended
        return self._step([None] * self.channels, np.zeros(self.channels, np.int64), ending)

    def _merge(self, per_round):
        """Rounds of (segments, counts), each channel-major -> one channel-major tensor (one gather)."""
        counts = np.sum([n for _, n in per_round], axis=0)
        if len(per_round) == 1 or not counts.any():
            return (per_round[0][0] if len(per_round) == 1 else self._empty()), counts
        allseg = torch.cat([s for s, _ in per_round])
        base, order = 0, [[] for _ in range(self.channels)]
        for _, n in per_round:
            first = base + track_table(n)
            for c in np.nonzero(n)[0]:
                order[c].append(np.arange(first[c], first[c + 1]))
            base = int(first[-1])
        order = np.concatenate([a for per in order for a in per])
        return allseg[torch.from_numpy(order).to(self.device)], counts

    def _step(self, pieces, lens, ending):
        C, c = self.channels, self.settings
        counts = np.zeros(C, np.int64)
        if not lens.any() and not ending.any():
            return self._empty(), counts
        n_fft, hop, n_frames = int(c["n_fft"]), int(c["hop_len"]), int(c["n_frames"])
        parts, starts, blen, pos = [], np.zeros(C, np.int64), np.zeros(C, np.int64), 0
        for ch in range(C):
            k = self._carry[ch]
            starts[ch] = pos
            if k is not None and k.numel():
                parts.append(k)
                pos += k.numel()
            if lens[ch]:
                parts.append(pieces[ch])
                pos += int(lens[ch])
            blen[ch] = pos - starts[ch]
        # the carried samples of every channel and the new chunks in one buffer (one copy): the carries become views of
        # THIS bank, so the last step's bank is released
        bank = torch.cat(parts) if parts else torch.zeros(1, dtype=torch.float32, device=self.device)
        self.seen += lens
        self.ended |= ending
        new_frames = np.array([frames_ready(self.seen[ch], self.ended[ch], n_fft, hop) for ch in range(C)], np.int64)
        new_frames = np.maximum(new_frames, self.frames)          # (an ended stream's count never changes again)
        new_segs = np.array([segments_ready(f, n_frames, self.step) for f in new_frames], np.int64)
        segs = self._empty()
        if (new_frames > self.frames).any():
            if self._ring is None:
                self._ring = torch.zeros((C, int(c["n_mels"]), self.R), dtype=torch.float32, device=self.device)
            ops.stream_logmel(bank, starts, blen, self.base, self.seen, self.ended, self.frames, new_frames, self._ring,
                              c["fs"], n_fft, c["win_len"], hop, c["n_mels"])
            self.launches += 1
            if self.frames_log is not None:
                for ch in np.nonzero(new_frames > self.frames)[0]:
                    cols = torch.arange(int(self.frames[ch]), int(new_frames[ch]), device=self.device) & (self.R - 1)
                    self.frames_log[ch].append(self._ring[ch][:, cols])
            if (new_segs > self.segs).any():
                segs = ops.stream_segments(self._ring, self.segs, new_segs, n_frames, self.step)
                self.launches += 1
                counts = new_segs - self.segs
        for ch in range(C):
            if self.ended[ch]:
                self._carry[ch], self.base[ch] = None, self.seen[ch]
            elif blen[ch]:
                keep = keep_from(new_frames[ch], self.seen[ch], n_fft, hop)
                lo = int(starts[ch] + keep - self.base[ch])
                self._carry[ch], self.base[ch] = bank[lo:int(starts[ch] + blen[ch])], keep
        self.frames, self.segs = new_frames, new_segs
        return segs, counts


class StreamMonitor:
    """What is playing on each of `channels` live feeds, against any form of FingerprintLibrary (flat, compact,
    thinned).

    push(chunks) -> per channel, the windows that became due: the dicts identify_windows returns ({start_s, end_s,
    segment_start_s, matches}) plus "channel".  For each channel the windows reported up to any moment are a prefix of
    library.window_items(segments, samples, ...) of the finished stream, each reported once; while the stream is open
    window w is reported by the first push after which window_items(segments so far, samples so far) lists it with its
    full length (`per_window` segments) -- not as soon as its segments exist: at the default settings the segments of
    the window that starts at 12 s are complete 384 samples before identify_windows would count that window (after
    239 616 of 240 000 samples).  end(channel) reports the rest, the short windows at the stream's end included.

    Per channel the monitor keeps the fingerprint rows and hit ids from the first row of the next window that has not
    been reported, and the windows it reported (timeline()).  max_chunk_s sizes the spectrogram ring; longer chunks are
    fed in pieces.  All work runs on the current stream.

    query_stride = Q > 1 (a flat library that keeps every row): a channel keeps only the segments whose index in the
    channel's stream is a multiple of Q.  push() hands only those to the model (1 / Q of its work); push_rows() still
    takes the channel's dense rows and files the kept ones, the others are never read.  The windows are scheduled on
    the dense segment counts as without it, each one's item is library.kept_items of it, and what is reported is
    identify_windows(query_stride=Q) of the finished stream.

    tempo, tempo_step (identify()'s arguments; a flat library that keeps every row, query_stride 1): the feeds may play
    faster or slower than the catalogue.  The ratio grid is fixed here, tempo_nums = tempo_ratios(tempo, per_window,
    tempo_step), with tempo_step the step actually used, and every window -- the short ones at a stream's end too -- is
    searched over it: what is reported is identify_windows(tempo=tempo, tempo_step=mon.tempo_step) of the finished
    stream, each match with its "tempo" and "tempo_num", and timeline() follows the slope.

    tempo_lock = N >= 1 (with tempo): a station's speed is constant for hours, so a channel whose last N windows agreed
    is searched over three ratios instead of the whole grid.  Per channel, host state: `lock`,
    None or (track, j) with j an index into tempo_nums, and `run`, the most recent consecutive windows with a match, each
    as (track, j).  A window of an unlocked channel is searched over the whole grid; one of a channel locked at (t, j)
    over tempo_nums[max(0, j - 1) : j + 2], and if that finds nothing or another best track than t the channel unlocks,
    its run is cleared and the SAME window is identified again over the whole grid (that result is reported).  After a
    window's final result: no match clears run and lock; else its best match (t', j') extends run if run's last element
    has track t' and an index within 1 of j', otherwise run = [(t', j')]; once len(run) >= N, lock = (t', j') -- a locked
    channel follows a drift of one grid step per window.  The windows of one channel are identified in order, each under
    the state its predecessors left: a push in which some channel has d due windows runs d rounds, each one
    ops.identify_tempo_items launch for that round's windows of all channels (unlocked ones with the whole grid as their
    window) plus at most one whole-grid launch for the windows that unlocked -- so what is reported depends on the
    stream, not on how it was cut into pushes.  Every window then also carries "locked": whether its reported result
    came from the three-ratio search; tempo_stats counts the windows reported from a whole-grid search ("full"), from a
    three-ratio one ("locked") and those identified twice ("redone", which are among "full").  reset() clears a
    channel's lock and run."""

    def __init__(self, library, channels, window_s=3.0, hop_s=1.0, top=5, k_probe=20, min_overlap=None,
                 max_chunk_s=1.0, query_stride=1, tempo=None, tempo_step=None, tempo_lock=0):
        self.library = library
        library._need_tempo_form("StreamMonitor", tempo)
        self.query_stride = library._need_stride_form("StreamMonitor", query_stride, tempo)
        if int(tempo_lock) != tempo_lock or int(tempo_lock) < 0:
            raise ValueError(f"tempo_lock={tempo_lock} must be a whole number of windows, 0 for no lock")
        if int(tempo_lock) and tempo is None:
            raise ValueError(f"tempo_lock={tempo_lock} needs tempo: it locks a channel to a ratio of the tempo search")
        c = library.settings
        _check_settings(c)
        self.channels = int(channels)
        if self.channels < 1:
            raise ValueError(f"channels={channels} must be at least 1")
        self.window_s, self.hop_s = float(window_s), float(hop_s)
        if not (self.window_s > 0 and self.hop_s > 0):
            raise ValueError("window_s and hop_s must be positive")
        self.top, self.k_probe, self.min_overlap = int(top), int(k_probe), min_overlap
        self.per_window = n_segments(int(round(self.window_s * c["fs"])), c)
        if self.per_window < 1:
            raise ValueError(f"a window of {window_s} s is shorter than one segment")
        self.per_kept = -(-self.per_window // self.query_stride)      # the most kept rows a window holds
        library._check_item_len(self.per_kept, self.k_probe)
        self.tempo, self.tempo_nums, self.tempo_step, self.tempo_lock = tempo, None, None, int(tempo_lock)
        if tempo is not None:
            self.tempo_step = max(1, ops.IDENTIFY_TEMPO_DEN // self.per_window) if tempo_step is None else int(tempo_step)
            self.tempo_nums = tempo_ratios(tempo, self.per_window, self.tempo_step)
            self.tempo_stats = {"full": 0, "locked": 0, "redone": 0}
        self._lock = [None] * self.channels       # tempo_lock: (track, index into tempo_nums) or None
        self._run = [[] for _ in range(self.channels)]
        self.front = StreamFrontEnd(c, self.channels, library.device, max_chunk_s)
        C = self.channels
        self._mode = [None] * C                  # None, "audio" (push) or "rows" (push_rows)
        self._closed = np.zeros(C, bool)
        self._n_rows = np.zeros(C, np.int64)     # segments so far (dense, whatever the query stride)
        self._samples = np.zeros(C, np.int64)    # rows-fed channels: the samples the caller said it has seen
        self._n_win = np.zeros(C, np.int64)      # windows reported
        self._windows = [[] for _ in range(C)]
        # the rows and hits still needed, channel by channel in ONE pair of tensors: channel c's are
        # [_first[c], _first[c + 1]), the first of them is row _row0[c] of the channel; _stale[c] of them are no longer
        # needed and go at the next ingest (one gather per push, whatever the number of channels).  These count KEPT
        # rows: kept row c of a channel is its segment c * query_stride
        self._q = self._ids = None
        self._first, self._row0, self._stale = np.zeros(C + 1, np.int64), np.zeros(C, np.int64), np.zeros(C, np.int64)

    # ---- feeding ---------------------------------------------------------------------------------------------------
    def _per_channel(self, items, what):
        items = list(items)
        if len(items) != self.channels:
            raise ValueError(f"{what}: {len(items)} entries for {self.channels} channels (None or empty: nothing for "
                             "that channel)")
        return items

    def _claim(self, ch, mode):
        if self._closed[ch]:
            raise ValueError(f"channel {ch} has ended; reset({ch}) starts a new stream on it")
        if self._mode[ch] not in (None, mode):
            raise ValueError(f"channel {ch} is fed with {'push_rows' if mode == 'audio' else 'push'} already")
        self._mode[ch] = mode

    def _kept_of(self, ch, n):
        """Of channel ch's next n segments, behind its _n_rows[ch] earlier ones, those whose index in the channel's
        stream is a multiple of query_stride -> their positions among the n."""
        lo, Q = int(self._n_rows[ch]), self.query_stride
        return np.arange(-(-lo // Q) * Q, lo + int(n), Q) - lo

    def _kept(self, packed, counts):
        """Of the new segments of all channels, packed channel by channel (counts[ch] of channel ch), the kept ones, by
        one gather -> (kept, kept counts).  At query_stride 1: (packed, counts)."""
        if self.query_stride == 1:
            return packed, counts
        base, pick, kept = track_table(counts), [], np.zeros(self.channels, np.int64)
        for ch in np.nonzero(counts)[0]:
            idx = self._kept_of(ch, counts[ch])
            pick.append(base[ch] + idx)
            kept[ch] = idx.size
        pick = np.concatenate(pick).astype(np.int64) if pick else np.zeros(0, np.int64)
        return packed[torch.from_numpy(pick).to(packed.device)], kept

    def push(self, chunks, fs=None):
        """One 1-D waveform per channel (tensor or array; empty or None: nothing for that channel), at `fs` (default
        settings['fs']).  Other rates go through ops.resample, chunk by chunk: that is NOT the resampling of the whole
        stream (every chunk is filtered as if silence surrounded it), so the bit-exact contract holds for
        fs == settings['fs'] only.  -> per channel, the list of new windows.  A push in which nothing becomes ready
        launches nothing."""
        chunks = self._per_channel(chunks, "push")
        lib, fs0 = self.library, int(self.library.settings["fs"])
        waves = [None] * self.channels
        for ch, w in enumerate(chunks):
            if w is None:
                continue
            w = torch.as_tensor(w)
            if w.dim() != 1:
                raise ValueError(f"push: channel {ch}'s chunk must be 1-D, not {tuple(w.shape)}")
            if w.numel():
                self._claim(ch, "audio")
                waves[ch] = w.to(lib.device, torch.float32)
        live = [ch for ch in range(self.channels) if waves[ch] is not None]
        if not live:
            return [[] for _ in range(self.channels)]
        if fs is not None and int(fs) != fs0:
            lens = torch.tensor([waves[ch].numel() for ch in live], dtype=torch.int64)
            out, starts, out_lens = ops.resample(torch.cat([waves[ch] for ch in live]), torch.cumsum(lens, 0) - lens,
                                                 lens, int(fs), fs0)
            starts, out_lens = starts.cpu().tolist(), out_lens.cpu().tolist()
            for j, ch in enumerate(live):
                waves[ch] = out[starts[j]:starts[j] + out_lens[j]]
        segs, counts = self.front.push(waves)
        segs, kept = self._kept(segs, counts)
        rows = lib._embed(segs) if segs.shape[0] else None
        return self._advance(rows, counts, live, kept)

    def push_rows(self, rows_per_channel, samples=None):
        """The same scheduling from fingerprint rows the caller already has (its own embedder, or rows computed
        elsewhere): per channel a (n, 128) tensor of the channel's NEXT n rows, or None.  samples: per channel, the
        samples of the stream seen so far (None: the fewest samples that many segments need, samples_lower_bound --
        windows are then reported as early as they can be told to be final).  -> per channel, the list of new windows.
        With a query_stride the rows given stay the channel's dense ones; only the kept ones are read."""
        items = self._per_channel(rows_per_channel, "push_rows")
        samples = None if samples is None else self._per_channel(samples, "push_rows")
        dev, parts, counts, live = self.library.device, [], np.zeros(self.channels, np.int64), []
        kept = counts if self.query_stride == 1 else np.zeros(self.channels, np.int64)
        for ch, r in enumerate(items):
            if r is None:
                continue
            r = torch.as_tensor(r)
            if r.dim() != 2 or r.shape[1] != 128:
                raise ValueError(f"push_rows: channel {ch}'s rows must be (n, 128), not {tuple(r.shape)}")
            if r.shape[0]:
                self._claim(ch, "rows")
                counts[ch] = r.shape[0]
                if self.query_stride != 1:
                    idx = self._kept_of(ch, r.shape[0])
                    r, kept[ch] = r[torch.from_numpy(idx).to(r.device)], idx.size
                parts.append(r.to(dev, torch.float32))
                live.append(ch)
        for ch in range(self.channels):
            if samples is not None and samples[ch] is not None and self._mode[ch] != "audio":
                self._claim(ch, "rows")
                self._samples[ch] = max(int(self._samples[ch]), int(samples[ch]))
                if ch not in live:
                    live.append(ch)
        if not live:
            return [[] for _ in range(self.channels)]
        return self._advance(torch.cat(parts).contiguous() if parts else None, counts, live, kept)

    def end(self, channel, n_samples=None):
        """The stream on `channel` (an index or several) has ended: flushes the frames, segments and windows that were
        waiting for more audio and returns the new windows (per channel for several, else that channel's list).  A
        channel fed with push_rows takes n_samples, the stream's final sample count (window_items needs it)."""
        many = not isinstance(channel, (int, np.integer))
        chans = [int(c) for c in channel] if many else [int(channel)]
        for ch in chans:
            if not 0 <= ch < self.channels:
                raise ValueError(f"channel {ch} not in [0, {self.channels})")
        chans = [ch for ch in chans if not self._closed[ch]]
        for ch in chans:
            if self._mode[ch] == "rows":
                if n_samples is None:
                    raise ValueError(f"end: channel {ch} was fed with push_rows and needs n_samples")
                if n_segments(int(n_samples), self.library.settings) != self._n_rows[ch]:
                    raise ValueError(f"end: a stream of {n_samples} samples has "
                                     f"{n_segments(int(n_samples), self.library.settings)} segments, channel {ch} was "
                                     f"fed {int(self._n_rows[ch])} rows")
                self._samples[ch] = int(n_samples)
        audio = [ch for ch in chans if self._mode[ch] != "rows"]
        segs, counts = self.front.end(audio)
        segs, kept = self._kept(segs, counts)
        rows = self.library._embed(segs) if segs.shape[0] else None
        self._closed[chans] = True
        out = self._advance(rows, counts, chans, kept)
        return out if many else out[chans[0]] if chans else []

    def reset(self, channel):
        """Start a new stream on `channel`: its audio state, rows and reported windows are dropped."""
        ch = int(channel)
        self.front.reset(ch)
        self._mode[ch], self._closed[ch] = None, False
        self._n_rows[ch] = self._samples[ch] = self._n_win[ch] = 0
        self._windows[ch] = []
        self._lock[ch], self._run[ch] = None, []
        self._stale[ch] = self._first[ch + 1] - self._first[ch]      # (its kept rows go at the next ingest)
        self._row0[ch] = -self._stale[ch]                            # so that the next row kept is row 0

    def timeline(self, channel, min_score=None):
        """library.timeline over the windows `channel` has reported so far."""
        return self.library.timeline(self._windows[int(channel)], min_score)

    def windows(self, channel):
        """The windows `channel` has reported so far."""
        return list(self._windows[int(channel)])

    # ---- scheduling ------------------------------------------------------------------------------------------------
    def _seen(self, ch):
        if self._mode[ch] == "rows":
            return max(int(self._samples[ch]), samples_lower_bound(int(self._n_rows[ch]), self.library.settings))
        return int(self.front.seen[ch])

    def _ingest(self, rows, counts):
        """Search the new rows (one launch sequence for all channels) and file them, and their hits, behind the rows
        each channel still keeps; drop the stale ones.  One gather for all channels."""
        lib, C = self.library, self.channels
        ids = lib._search_rows(rows, self.k_probe) if lib.n_rows else \
            torch.zeros((rows.shape[0], 0), dtype=torch.int64, device=rows.device)
        n_old = int(self._first[-1])
        new_first = n_old + track_table(counts)
        order = []
        for ch in range(C):
            order.append(np.arange(self._first[ch] + self._stale[ch], self._first[ch + 1]))
            order.append(np.arange(new_first[ch], new_first[ch + 1]))
        order = torch.from_numpy(np.concatenate(order).astype(np.int64)).to(rows.device)
        self._q = (torch.cat([self._q, rows]) if n_old else rows)[order]
        self._ids = (torch.cat([self._ids, ids]) if n_old else ids)[order]
        kept = np.diff(self._first) - self._stale + counts
        self._row0 += self._stale
        self._stale[:] = 0
        self._first = track_table(kept)

    def _advance(self, rows, counts, touched, kept):
        """File the new rows (kept[ch] of channel ch, of its counts[ch] new segments), find the windows that became due
        on the touched channels and identify them all in one launch."""
        lib, c, Q = self.library, self.library.settings, self.query_stride
        if rows is not None and rows.shape[0]:
            self._ingest(rows, kept)
        self._n_rows += counts
        seg_hop = self.front.step * int(c["hop_len"])
        due = []                                  # (channel, start_s, first row, rows)
        for ch in touched:
            starts, jrow, lens = window_items(int(self._n_rows[ch]), self._seen(ch), c, self.window_s, self.hop_s)
            w = int(self._n_win[ch])
            while w < len(starts) and (self._closed[ch] or lens[w] == self.per_window):
                due.append((ch, float(starts[w]), int(jrow[w]), int(lens[w])))
                w += 1
            self._n_win[ch] = w
            # rows before the next unreported window's first row are not needed again (kept rows: before ceil(nxt / Q))
            nxt = -(-int(round(w * self.hop_s * c["fs"])) // seg_hop)
            nxt = -(-nxt // Q)
            have = self._first[ch + 1] - self._first[ch]
            self._stale[ch] = have if self._closed[ch] else min(have, max(int(self._stale[ch]),
                                                                          nxt - int(self._row0[ch])))
        out = [[] for _ in range(self.channels)]
        if not due:
            return out
        # a window's item: its kept rows (at Q = 1 the window itself); one that holds none keeps its dense first segment
        krow, item_len = kept_items([j for _, _, j, _ in due], [n for _, _, _, n in due], Q)
        due = [(ch, s, int(k) * Q if n else j, n) for (ch, s, j, _), k, n in zip(due, krow, item_len)]
        item_row = np.array([self._first[ch] + k - self._row0[ch] for (ch, _, _, _), k in zip(due, krow)], np.int64)
        item_row[item_len == 0] = 0
        locked = None
        if not (lib.n_rows and self._q is not None and item_len.any()):
            res = [[] for _ in due]
            if self.tempo is not None:
                self.tempo_stats["full"] += len(due)
            if self.tempo_lock:
                locked = [False] * len(due)
                for ch in {d[0] for d in due}:
                    self._lock[ch], self._run[ch] = None, []
        elif self.tempo is None:
            res = lib._identify_items(self._q, self._ids, item_row, item_len, self.top, self.min_overlap,
                                      max_len=self.per_kept, q_stride=Q)
        elif not self.tempo_lock:
            res = lib._identify_items(self._q, self._ids, item_row, item_len, self.top, self.min_overlap,
                                      max_len=self.per_kept, tempo=self.tempo, tempo_step=self.tempo_step)
            self.tempo_stats["full"] += len(due)
        else:
            res, locked = self._identify_locked([d[0] for d in due], item_row, item_len)
        seg_s = lib.segment_s
        for i, ((ch, s, j, _), m) in enumerate(zip(due, res)):
            win = {"start_s": s, "end_s": s + self.window_s, "segment_start_s": j * seg_s, "matches": m, "channel": ch}
            if locked is not None:
                win["locked"] = locked[i]
            self._windows[ch].append(win)
            out[ch].append(win)
        return out

    # ---- the tempo lock ----------------------------------------------------------------------------------------------
    def _identify_locked(self, chans, item_row, item_len):
        """The due windows (chans[i]: window i's channel; a channel's windows in order) under the lock rule stated at the
        top of the class -> (per-window matches, per-window whether the reported result came from the locked search).
        Round r identifies the r-th due window of every channel that has one: one launch with a ratio window per item,
        then at most one over the whole grid for the windows that unlocked."""
        G, R, N = self.tempo_nums, len(self.tempo_nums), self.tempo_lock
        per_channel = {}
        for i, ch in enumerate(chans):
            per_channel.setdefault(ch, []).append(i)
        res, locked = [None] * len(chans), [False] * len(chans)

        def launch(sel, lo, cnt):
            return self.library._identify_items(self._q, self._ids, item_row[sel], item_len[sel], self.top,
                                                self.min_overlap, max_len=self.per_kept, tempo=self.tempo,
                                                tempo_step=self.tempo_step, ratio_window=(lo, cnt))
        for r in range(max(len(v) for v in per_channel.values())):
            sel = np.array([v[r] for v in per_channel.values() if len(v) > r], np.int64)
            lo, cnt = np.zeros(len(sel), np.int64), np.full(len(sel), R, np.int64)
            for n, i in enumerate(sel):
                lock = self._lock[chans[i]]
                if lock is not None:
                    lo[n] = max(0, lock[1] - 1)
                    cnt[n] = min(R, lock[1] + 2) - lo[n]
            redo = []
            for n, (i, m) in enumerate(zip(sel, launch(sel, lo, cnt))):
                ch = chans[i]
                lock = self._lock[ch]
                if lock is not None and (not m or m[0]["track"] != lock[0]):
                    self._lock[ch], self._run[ch] = None, []
                    redo.append(i)
                else:
                    res[i], locked[i] = m, lock is not None
            if redo:
                redo = np.array(redo, np.int64)
                for i, m in zip(redo, launch(redo, np.zeros(len(redo), np.int64), np.full(len(redo), R, np.int64))):
                    res[i] = m
                self.tempo_stats["redone"] += len(redo)
            for i in sel:
                ch, m = chans[i], res[i]
                self.tempo_stats["locked" if locked[i] else "full"] += 1
                if not m:
                    self._lock[ch], self._run[ch] = None, []
                    continue
                here = (m[0]["track"], int(np.searchsorted(G, m[0]["tempo_num"])))
                run = self._run[ch]
                if run and run[-1][0] == here[0] and abs(run[-1][1] - here[1]) <= 1:
                    run.append(here)
                    del run[:-N]
                else:
                    run[:] = [here]
                if len(run) >= N:
                    self._lock[ch] = here
        return res, locked
