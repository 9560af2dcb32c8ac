"""Brute-force restatements for the stream front end (grafp_amd/monitor.py, csrc/stream_frontend.hip) and a CPU stand-in
for its two launches, so that the host state machine runs without a GPU.

read_positions enumerates what the offline log-mel kernel reads for one frame (csrc/logmel_core.h: window sample t of
frame f is position f * hop + t - n_fft/2, reflected at 0 and at T as torch.stft(center=True, pad_mode='reflect')
does).  FakeFrontEnd replaces ops.stream_logmel / ops.stream_segments: it runs the real host checks
(ops.stream_logmel_plan), then checks by enumeration that every sample a due frame reads is in the channel's buffer AND is
the right sample of the whole stream -- the carry never dropped or misplaced it."""
import numpy as np
import torch

from grafp_amd import ops

CHUNK_CYCLE = (0, 1, 511, 512, 513, 1535, 4096)


def read_positions(f, n_fft, hop, T=None):
    """Positions of the signal frame f reads; T=None: a stream whose end is unknown (no reflection there)."""
    half = n_fft // 2
    p = f * hop + np.arange(n_fft, dtype=np.int64) - half
    p = np.abs(p)
    if T is not None:
        p = np.where(p >= T, 2 * (T - 1) - p, p)
    return p


def random_chunks(total, seed, big=9000):
    """Chunk sizes that sum to `total`: zeros, single samples and sizes up to `big`, seeded."""
    rng = np.random.RandomState(seed)
    out, left = [], int(total)
    while left:
        kind = rng.randint(0, 6)
        n = 0 if kind == 0 else 1 if kind == 1 else int(rng.randint(2, big))
        n = min(n, left)
        out.append(n)
        left -= n
    return out


def cycle_chunks(total, phase):
    """Chunk sizes cycling through CHUNK_CYCLE from `phase` on, summing to `total`."""
    out, left, i = [], int(total), int(phase)
    while left:
        n = min(CHUNK_CYCLE[i % len(CHUNK_CYCLE)], left)
        out.append(n)
        left -= n
        i += 1
    return out


class FakeFrontEnd:
    """Stand-ins for ops.stream_logmel and ops.stream_segments on CPU tensors.  whole[c]: channel c's full stream (numpy
    f32), so that the buffer's CONTENT can be checked against the positions a frame reads.  Collects the frame and
    segment ranges asked for."""

    def __init__(self, whole, n_fft, hop):
        self.whole, self.n_fft, self.hop = whole, n_fft, hop
        self.frame_ranges = [[] for _ in whole]
        self.seg_ranges = [[] for _ in whole]
        self.calls = 0

    def stream_logmel(self, bank, starts, lengths, base, seen, ended, frame_lo, frame_hi, ring, fs, n_fft, win_len, hop,
                      n_mels):
        self.calls += 1
        C, R = ring.shape[0], ring.shape[2]
        plan = ops.stream_logmel_plan(C, R, bank.numel(), starts, lengths, base, seen, ended, frame_lo, frame_hi, n_fft,
                                      hop)
        if plan is None:
            return 0
        st, ln, bs, lo, hi, first = plan
        buf = bank.numpy()
        for c in range(C):
            for f in range(int(lo[c]), int(hi[c])):
                p = read_positions(f, n_fft, hop, int(seen[c]) if ended[c] else None)
                assert p.min() >= bs[c] and p.max() < bs[c] + ln[c], (c, f, int(p.min()), int(p.max()), int(bs[c]), int(ln[c]))
                assert np.array_equal(buf[st[c] + p - bs[c]], self.whole[c][p]), (c, f)
            if hi[c] > lo[c]:
                self.frame_ranges[c].append((int(lo[c]), int(hi[c])))
        return int(first[-1])

    def stream_segments(self, ring, seg_lo, seg_hi, size, step):
        self.calls += 1
        n = 0
        for c, (a, b) in enumerate(zip(seg_lo, seg_hi)):
            if b > a:
                self.seg_ranges[c].append((int(a), int(b)))
                n += int(b - a)
        return torch.zeros((n, ring.shape[1], size))

    def install(self, monkeypatch):
        monkeypatch.setattr(ops, "stream_logmel", self.stream_logmel)
        monkeypatch.setattr(ops, "stream_segments", self.stream_segments)
        return self
