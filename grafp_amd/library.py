"""Identify recordings against a track-indexed fingerprint library.

A FingerprintLibrary holds the fingerprints of whole tracks resident in an ops.FlatL2Index (bf16 pre-filter, exact
results), the track table (track t owns rows [first[t], first[t+1])), the track names and the segmentation settings the
rows were cut with.  identify() takes recordings nobody has labelled and says which tracks they are and where in each
they start: log-mel and segments on the device, one batched embed, one batched search, then one ops.identify launch
(csrc/identify.hip) for all queries.  Unlike eval.py's row-level rerank (ops.seq_rerank), a candidate never reads
across a track boundary and the result is the best tracks, not the best rows."""
import hashlib
import json
import math
import os

import numpy as np
import torch

from . import ops

SETTINGS = ("fs", "n_fft", "win_len", "hop_len", "n_mels", "n_frames", "overlap")
FORMAT = 1
# duplicate_groups' default score bar: a match at least this strong is shared audio.  Chosen from
# tests/test_gpu_selfmatch.py's trained-model case (the briefly trained model of tests/_retrieval_case.py, bf16 library,
# measured on MI355X): an exact copy scores 1.000, the pieces of a medley at 20 dB SNR 0.985 and 0.956, the strongest of
# the 77 unrelated pairs that pass the 3 s / 4-vote filters 0.832.  0.9 sits between the two, 0.07 above the unrelated.
DUPLICATE_MIN_SCORE = 0.9


def model_digest(model):
    """sha256 over the model's state_dict (names, dtypes, shapes and values, in name order)."""
    core = model.module if hasattr(model, "module") else model
    h = hashlib.sha256()
    for name, v in sorted(core.state_dict().items()):
        t = v.detach().cpu().contiguous()
        h.update(f"{name}|{t.dtype}|{tuple(t.shape)}|".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    return h.hexdigest()


def segment_step(settings):
    return int(settings["n_frames"] * (1 - settings["overlap"]))


def n_segments(n_samples, settings):
    """Segments GPUTransformNeuralfp._segments cuts from n_samples samples (1 + T // hop frames, windows of n_frames
    every `step` frames)."""
    frames = 1 + int(n_samples) // int(settings["hop_len"])
    if frames < settings["n_frames"]:
        return 0
    return (frames - int(settings["n_frames"])) // segment_step(settings) + 1


def segment_seconds(settings):
    """Seconds between the starts of two consecutive segments: step * hop_len / fs."""
    return segment_step(settings) * settings["hop_len"] / settings["fs"]


def window_items(n_seg_total, n_samples, settings, window_s=3.0, hop_s=1.0):
    """Items of identify_windows: a window of window_s seconds every hop_s seconds over a recording of n_samples
    samples whose n_seg_total segments are on the recording's own grid.  A window takes the segments that start at or
    after its start, as many as a window_s crop would have.  -> (start_s, item_row, item_len), one entry per window."""
    fs = float(settings["fs"])
    dur = n_samples / fs
    seg_hop = segment_step(settings) * int(settings["hop_len"])             # samples between segment starts
    per_window = n_segments(int(round(window_s * fs)), settings)
    n_win = 1 if dur <= window_s else int(math.floor((dur - window_s) / hop_s + 1e-9)) + 1
    starts, rows, lens = [], [], []
    for w in range(n_win):
        s0 = int(round(w * hop_s * fs))
        j0 = min(-(-s0 // seg_hop), n_seg_total)
        starts.append(w * hop_s)
        rows.append(j0)
        lens.append(max(0, min(per_window, n_seg_total - j0)))
    return np.array(starts, np.float64), np.array(rows, np.int64), np.array(lens, np.int32)


def _as_waveforms(tracks):
    """A DeviceAudioCorpus (-> every track and its file names), its .tracks(), or 1-D tensors / arrays."""
    from .data import DeviceAudioCorpus
    if isinstance(tracks, DeviceAudioCorpus):
        n = len(tracks)
        names = list(tracks.files) if tracks.files is not None else None
        return [tracks.track(i) for i in range(n)], names
    if isinstance(tracks, (np.ndarray, torch.Tensor)) and tracks.ndim == 1:
        tracks = [tracks]
    return list(tracks), None


class FingerprintLibrary:
    """Fingerprints of whole tracks, resident on one device, with the table that says which rows are which track."""

    def __init__(self, model, settings, rows, first, names=None, precision="bf16", device=None):
        if precision not in ("bf16", "f32"):
            raise ValueError(f"precision must be 'bf16' or 'f32', not {precision!r}")
        self.model = model
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        self.settings = {k: settings[k] for k in SETTINGS}
        self.precision = precision
        self._chunks, self._rows, self._index = [], None, None
        self.first = np.zeros(1, np.int64)
        self.names = []
        if rows is not None:
            self._append(rows, first, names)

    # ---- sizes -----------------------------------------------------------------------------------------------
    @property
    def step(self):
        return segment_step(self.settings)

    @property
    def segment_s(self):
        return segment_seconds(self.settings)

    @property
    def n_tracks(self):
        return len(self.first) - 1

    @property
    def n_rows(self):
        return int(self.first[-1])

    def rows(self):
        """The resident (n_rows, 128) f32 fingerprints."""
        if self._rows is None:
            self._rows = (self._chunks[0] if len(self._chunks) == 1 else
                          torch.cat(self._chunks) if self._chunks else torch.zeros((0, 128), device=self.device))
            self._chunks = [self._rows] if self._chunks else []
        return self._rows

    @property
    def index(self):
        """The ops.FlatL2Index over rows() (made on first use; it shares the rows tensor)."""
        if self._index is None:
            self._index = ops.FlatL2Index(d=128, device=self.device)
            self._index.add(self.rows())
        return self._index

    def _append(self, rows, first, names):
        first = np.asarray(first, np.int64).reshape(-1)
        rows = torch.as_tensor(rows).to(self.device, torch.float32).reshape(-1, 128)
        ops.check_track_table(first, rows.shape[0])
        T = len(first) - 1
        names = [str(v) for v in names] if names is not None else [f"track{self.n_tracks + i}" for i in range(T)]
        if len(names) != T:
            raise ValueError(f"{len(names)} names for {T} tracks")
        if rows.shape[0]:
            self._chunks.append(rows.contiguous())
            self._rows, self._index = None, None
        self.first = np.concatenate([self.first, self.first[-1] + first[1:]])
        self.names += names

    # ---- fingerprinting --------------------------------------------------------------------------------------
    def _autocast(self):
        if self.precision == "bf16":
            return torch.autocast("cuda", dtype=torch.bfloat16)
        return torch.autocast("cuda", enabled=False)

    def _embed(self, segs):
        core = self.model.module if hasattr(self.model, "module") else self.model
        was = core.training
        core.eval()
        try:
            with torch.no_grad(), self._autocast():
                return core.embed(segs)[1].float()
        finally:
            core.train(was)

    def segments(self, wav):
        """Log-mel segments of one recording at settings['fs'], exactly as GPUTransformNeuralfp._segments cuts them:
        (n_seg, n_mels, n_frames)."""
        c = self.settings
        x = torch.as_tensor(wav).to(self.device, torch.float32).reshape(-1)
        if x.numel() == 0:
            return torch.empty((0, c["n_mels"], c["n_frames"]), device=self.device)
        spec = ops.logmel(x, c["fs"], c["n_fft"], c["win_len"], c["hop_len"], c["n_mels"])
        return ops.unfold_segments(spec, c["n_frames"], self.step)

    def _fingerprint_tracks(self, waves, max_segments):
        """Segments of consecutive tracks packed into model calls as fpdb._embed_stream packs them in eval mode (a call
        once at least max_segments segments are pending) -> (rows, per-track row counts)."""
        out, counts, pend, n_pend = [], [], [], 0

        def flush():
            nonlocal pend, n_pend
            if n_pend:
                out.append(self._embed(torch.cat(pend, dim=0)))
            pend, n_pend = [], 0

        for w in waves:
            segs = self.segments(w)
            counts.append(segs.shape[0])
            pend.append(segs)
            n_pend += segs.shape[0]
            if n_pend >= max_segments:
                flush()
        flush()
        rows = torch.cat(out, dim=0) if out else torch.zeros((0, 128), device=self.device)
        return rows, counts

    @classmethod
    def build(cls, model, tracks, cfg, names=None, precision="bf16", max_segments=4096):
        """Fingerprint whole tracks (a DeviceAudioCorpus, its .tracks(), or 1-D tensors / arrays at cfg['fs']) into a
        new library.  Tracks shorter than one segment get no rows: they stay in the table and never match."""
        lib = cls(model, cfg, None, None, precision=precision)
        lib.add(tracks, names=names, max_segments=max_segments)
        return lib

    def add(self, tracks, names=None, max_segments=4096):
        """Append tracks (as for build) to the library."""
        waves, own = _as_waveforms(tracks)
        names = names if names is not None else own
        rows, counts = self._fingerprint_tracks(waves, int(max_segments))
        self._append(rows, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), names)
        return self

    # ---- files -----------------------------------------------------------------------------------------------
    def save(self, out_dir):
        """library.mm + library_shape.npy (the reference's memmap format: eval.load_memmap_data reads them),
        library_tracks.npy (the track table, int64) and library.json (names, settings, precision, model digest)."""
        from .fpdb import _write_memmap
        os.makedirs(out_dir, exist_ok=True)
        _write_memmap(os.path.join(out_dir, "library"), self.rows().cpu().numpy().reshape(-1, 128))
        np.save(os.path.join(out_dir, "library_tracks.npy"), self.first.astype(np.int64))
        meta = {"format": FORMAT, "names": self.names, "settings": self.settings, "precision": self.precision,
                "model_digest": model_digest(self.model), "n_rows": self.n_rows, "n_tracks": self.n_tracks}
        with open(os.path.join(out_dir, "library.json"), "w") as f:
            json.dump(meta, f, indent=1)

    @classmethod
    def load(cls, lib_dir, model, device=None, force=False):
        """A library written by save().  Refuses a model whose state_dict digest differs from the one the rows were
        made with, unless force=True."""
        with open(os.path.join(lib_dir, "library.json")) as f:
            meta = json.load(f)
        if meta.get("format") != FORMAT:
            raise ValueError(f"{lib_dir}: library format {meta.get('format')} is not {FORMAT}")
        if not force and model_digest(model) != meta["model_digest"]:
            raise ValueError(f"{lib_dir}: the library was fingerprinted with another model (state_dict digest "
                             f"{meta['model_digest'][:12]}...); pass force=True to use it anyway")
        first = np.load(os.path.join(lib_dir, "library_tracks.npy")).astype(np.int64)
        shape = tuple(int(v) for v in np.load(os.path.join(lib_dir, "library_shape.npy")))
        if shape[0] != int(first[-1]):
            raise ValueError(f"{lib_dir}: {shape[0]} rows but the track table covers {int(first[-1])}")
        rows = np.fromfile(os.path.join(lib_dir, "library.mm"), dtype=np.float32).reshape(shape) if shape[0] else \
            np.zeros((0, 128), np.float32)
        if device is not None:
            model = model.to(device)
        return cls(model, meta["settings"], torch.from_numpy(rows), first, meta["names"], meta["precision"], device)

    @classmethod
    def from_memmap(cls, db_dir, fname, track_rows, model, cfg, names=None, precision="f32"):
        """Attach a track table (rows per track, in order) to a database fpdb.create_dummy_db wrote as
        <fname>.mm + <fname>_shape.npy.  precision: how the queries are fingerprinted (create_dummy_db runs the model
        without autocast: f32)."""
        from .eval import PartedRows, load_memmap_data
        data, shape = load_memmap_data(db_dir, fname, display=False)
        rows = np.concatenate([np.asarray(p) for p in data.parts]) if isinstance(data, PartedRows) else np.asarray(data)
        counts = np.asarray(track_rows, np.int64).reshape(-1)
        if (counts < 0).any() or int(counts.sum()) != int(shape[0]):
            raise ValueError(f"track_rows sum to {int(counts.sum())}, the database holds {int(shape[0])} rows")
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return cls(model, cfg, torch.from_numpy(np.ascontiguousarray(rows, np.float32)), first, names, precision)

    # ---- queries ---------------------------------------------------------------------------------------------
    def _load_queries(self, queries, fs):
        """-> list of 1-D device waveforms at settings['fs']."""
        from .data import read_audio
        fs0 = int(self.settings["fs"])
        if isinstance(queries, str):
            queries = [queries]
        elif isinstance(queries, (np.ndarray, torch.Tensor)):
            queries = [queries] if queries.ndim <= 1 else list(queries)
        waves, rates = [], []
        for q in queries:
            if isinstance(q, str):
                a, r = read_audio(q, fs0 if fs is None else fs)
            else:
                a, r = q, (fs0 if fs is None else fs)
            waves.append(torch.as_tensor(np.asarray(a, np.float32) if isinstance(a, np.ndarray) else a)
                         .to(self.device, torch.float32).reshape(-1))
            rates.append(int(r))
        for r in sorted(set(rates)):
            if r == fs0:
                continue
            ids = [i for i, v in enumerate(rates) if v == r and waves[i].numel()]
            if not ids:
                continue
            lens = torch.tensor([waves[i].numel() for i in ids], dtype=torch.int64)
            bank = torch.cat([waves[i] for i in ids])
            out, starts, out_lens = ops.resample(bank, torch.cumsum(lens, 0) - lens, lens, r, fs0)
            starts, out_lens = starts.cpu().tolist(), out_lens.cpu().tolist()
            for j, i in enumerate(ids):
                waves[i] = out[starts[j]:starts[j] + out_lens[j]]
        return waves

    def _search_and_identify(self, segs, item_row, item_len, top, k_probe, min_overlap):
        """One batched embed + search of all segments, one ops.identify launch for all items -> per-item lists."""
        n_items = len(item_row)
        if n_items == 0 or segs.shape[0] == 0 or self.n_rows == 0 or int(np.max(item_len, initial=0)) == 0:
            return [[] for _ in range(n_items)]
        max_len = int(np.max(item_len))
        if max_len > ops.IDENTIFY_MAX_LEN or max_len * k_probe > ops.IDENTIFY_MAX_KEYS:
            raise ValueError(f"a query of {max_len} segments ({max_len * self.segment_s:.1f} s) with k_probe={k_probe} "
                             f"exceeds {ops.IDENTIFY_MAX_LEN} segments / {ops.IDENTIFY_MAX_KEYS} hits per item: use "
                             "identify_windows for long recordings")
        q = self._embed(segs)
        k = min(int(k_probe), self.n_rows)
        _, ids = self.index.search(q, k)
        dev = self.device
        tr, off, sc, vo = ops.identify(self.rows(), torch.from_numpy(self.first).to(dev), q, ids,
                                       torch.from_numpy(np.asarray(item_row, np.int64)).to(dev),
                                       torch.from_numpy(np.asarray(item_len, np.int32)).to(dev), top=top,
                                       min_overlap=min_overlap, max_len=max_len)
        tr, off, sc, vo = (t.cpu().numpy() for t in (tr, off, sc, vo))
        step, hop, fs = self.step, self.settings["hop_len"], self.settings["fs"]
        out = []
        for i in range(n_items):
            res = []
            for j in range(top):
                t = int(tr[i, j])
                if t < 0:
                    break
                res.append({"track": t, "name": self.names[t], "offset": int(off[i, j]),
                            "offset_s": int(off[i, j]) * step * hop / fs, "score": float(sc[i, j]),
                            "votes": int(vo[i, j])})
            out.append(res)
        return out

    def identify(self, queries, fs=None, top=5, k_probe=20, min_overlap=None):
        """queries: one waveform, a list of ragged waveforms, or file paths; at `fs` (default settings['fs']; other rates
        are resampled on the device).  -> per query, a list of matches {track, name, offset, offset_s, score, votes},
        best first.  offset_s = offset * step * hop_len / fs is where the query's first segment sits in the track.  A
        query shorter than one segment gives an empty list."""
        single = isinstance(queries, (str, np.ndarray, torch.Tensor)) and (
            isinstance(queries, str) or torch.as_tensor(queries).dim() == 1)
        waves = self._load_queries(queries, fs)
        segs = [self.segments(w) for w in waves]
        lens = np.array([s.shape[0] for s in segs], np.int32)
        rows = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
        allsegs = torch.cat(segs, dim=0) if segs else torch.empty((0,), device=self.device)
        res = self._search_and_identify(allsegs, rows, lens, int(top), int(k_probe), min_overlap)
        return res[0] if single and len(res) == 1 else res

    def identify_windows(self, recording, window_s=3.0, hop_s=1.0, fs=None, top=5, k_probe=20, min_overlap=None):
        """A long recording cut into items of window_s seconds every hop_s seconds.  The recording is segmented,
        fingerprinted and searched once; all windows are identified in one launch.  -> per window
        {start_s, end_s, segment_start_s, matches}; segment_start_s is where the window's first segment starts in the
        recording (the time its matches' offset_s refers to)."""
        wave = self._load_queries([recording], fs)[0]
        segs = self.segments(wave)
        starts, rows, lens = window_items(segs.shape[0], wave.numel(), self.settings, window_s, hop_s)
        res = self._search_and_identify(segs, rows, lens, int(top), int(k_probe), min_overlap)
        seg_s = self.segment_s
        return [{"start_s": float(s), "end_s": float(s) + window_s, "segment_start_s": int(r) * seg_s, "matches": m}
                for s, r, m in zip(starts, rows, res)]

    def timeline(self, windows, min_score=None):
        """What played when: consecutive windows whose best match is the same track at a consistent position (the
        track offset minus the window's segment start agrees within one segment hop) merge into one span.
        -> list of {start_s, end_s, track, name, track_offset_s (the track position at start_s), score (mean)}."""
        spans, seg_s = [], self.segment_s
        for w in windows:
            if not w["matches"] or (min_score is not None and w["matches"][0]["score"] < min_score):
                continue
            m = w["matches"][0]
            delta = m["offset_s"] - w["segment_start_s"]              # track time = recording time + delta
            last = spans[-1] if spans else None
            if (last is not None and last["track"] == m["track"] and abs(delta - last["_delta"]) <= seg_s + 1e-9
                    and w["start_s"] <= last["end_s"]):
                last["end_s"] = w["end_s"]
                last["_scores"].append(m["score"])
            else:
                spans.append({"start_s": w["start_s"], "end_s": w["end_s"], "track": m["track"], "name": m["name"],
                              "track_offset_s": w["start_s"] + delta, "_delta": delta, "_scores": [m["score"]]})
        for s in spans:
            s["score"] = float(np.mean(s.pop("_scores")))
            s.pop("_delta")
        return spans

    # ---- the catalog itself ------------------------------------------------------------------------------------
    def self_matches(self, k_probe=32, min_overlap_s=3.0, min_votes=4, min_score=None, top=8, tracks=None,
                     batch_rows=1 << 18):
        """Tracks that share audio: re-releases, compilations, edits, quotes.  The library's own rows (or only those of
        `tracks`) are searched against self.index in batches of about batch_rows rows, and each batch of source tracks
        goes through one ops.self_match launch.  -> list of {track_a, name_a, track_b, name_b, offset, a_start_s,
        b_start_s, overlap_s, coverage, score, votes}: track_a's audio from a_start_s reappears in track_b from
        b_start_s for overlap_s seconds; offset = delta in segments (row i of a sits on row i + offset of b), coverage =
        overlapping rows / rows of the shorter track, score = mean cosine over the span.  Ordered by track_a, then
        score descending, then track_b; both directions are reported (a -> b from a's rows, b -> a from b's).
        k_probe: hits per row.  At the default overlap of 0.9 a segment's nearest neighbours include its own track's
        next rows (a hop is a tenth of a segment), and those hits are dropped, so k_probe defaults to 32 (the most
        the kernel takes) rather than identify's 20.  min_overlap_s: the least span, in seconds of segment hops;
        min_votes: the least rows whose hits agree on the alignment; min_score: drop weaker matches (None: keep all).
        Memory: the kernel reads hits by library row, so the hits of the searched rows live in one (n_rows, k_probe)
        int64 tensor whatever `tracks` is (256 MB at 1 M rows and k_probe = 32); each batch also takes its own exactly
        sized workspace (ops.self_match_workspace_bytes: about 124 KB per 303-row source at k_probe = 32, min_votes 4)."""
        T, n = self.n_tracks, self.n_rows
        src = list(range(T)) if tracks is None else sorted({int(t) for t in tracks})
        if src and not 0 <= min(src) <= max(src) < T:
            raise ValueError(f"tracks must lie in [0, {T})")
        if n == 0 or T < 2 or not src:
            return []
        seg_s = self.segment_s
        min_overlap = max(1, int(math.ceil(float(min_overlap_s) / seg_s - 1e-9)))
        k = min(int(k_probe), n)
        rows, dev = self.rows(), self.device
        first_d = torch.from_numpy(self.first).to(dev)
        ids = torch.full((n, k), -1, dtype=torch.int64, device=dev)
        lens = np.diff(self.first)
        batches, cur, cur_rows = [], [], 0
        for t in src:
            cur.append(t)
            cur_rows += int(lens[t])
            if cur_rows >= batch_rows:
                batches.append(cur)
                cur, cur_rows = [], 0
        if cur:
            batches.append(cur)
        out = []
        for batch in batches:
            g = np.concatenate([np.arange(self.first[t], self.first[t + 1]) for t in batch]).astype(np.int64)
            if g.size:
                g_d = torch.from_numpy(g).to(dev)
                _, hit = self.index.search(rows[g_d], k)
                ids[g_d] = hit
            res = ops.self_match(rows, first_d, ids, tracks=torch.tensor(batch, dtype=torch.int64), top=int(top),
                                 min_votes=int(min_votes), min_overlap=min_overlap)
            b_, d_, lo_, m_, sc_, v_ = (x.cpu().numpy() for x in res)
            for s, a in enumerate(batch):
                for j in range(b_.shape[1]):
                    b = int(b_[s, j])
                    if b == -2:                                  # the op sizes the workspace exactly: never
                        raise RuntimeError(f"self_match: track {a} did not fit the workspace")
                    if b < 0:
                        break
                    sc = float(sc_[s, j])
                    if min_score is not None and sc < min_score:
                        continue
                    d, lo, m = int(d_[s, j]), int(lo_[s, j]), int(m_[s, j])
                    out.append({"track_a": a, "name_a": self.names[a], "track_b": b, "name_b": self.names[b],
                                "offset": d, "a_start_s": lo * seg_s, "b_start_s": (lo + d) * seg_s,
                                "overlap_s": m * seg_s, "coverage": m / max(1, min(int(lens[a]), int(lens[b]))),
                                "score": sc, "votes": int(v_[s, j])})
        return out

    @staticmethod
    def duplicate_groups(matches, min_coverage=0.9, min_score=DUPLICATE_MIN_SCORE):
        """Connected components of the tracks whose matches (from self_matches) cover at least min_coverage of the
        shorter track with at least min_score: duplicates, and chains of them.  -> list of sorted track lists (two or
        more tracks each), ordered by their first track.  Union-find on the host."""
        parent = {}

        def find(x):
            parent.setdefault(x, x)
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for m in matches:
            if m["coverage"] >= min_coverage and (min_score is None or m["score"] >= min_score):
                ra, rb = find(int(m["track_a"])), find(int(m["track_b"]))
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
        groups = {}
        for x in parent:
            groups.setdefault(find(x), []).append(x)
        return sorted((sorted(g) for g in groups.values() if len(g) > 1), key=lambda g: g[0])
