"""Identify recordings against a track-indexed fingerprint library.

A FingerprintLibrary holds the fingerprints of whole tracks resident in an ops.FlatL2Index (bf16 pre-filter, exact
results), the track table (track t owns rows [first[t], first[t+1])), the track names and the segmentation settings the
rows were cut with.  identify() takes recordings nobody has labelled and says which tracks they are and where in each
they start: log-mel and segments on the device, one batched embed, one batched search, then one ops.identify launch
(csrc/identify.hip) for all queries.  Unlike eval.py's row-level rerank (ops.seq_rerank), a candidate never reads
across a track boundary and the result is the best tracks, not the best rows.

A library has three forms, each a class of grafp_amd/_forms.py; it holds one form object, which answers whatever
depends on how the rows are held (the tensors, the index, the files, the ops).  The flat form above keeps every row as
f32 (plus the index's bf16 copy and norms: 772 bytes per row).  The compact form keeps IVF-PQ codes only -- per row M code bytes in row order, the list id, and the
grafp_amd.ivfpq.IVFPQIndex over them (the codes again in list order, the ids): 2 M + 20 bytes per row, 148 at M = 64 --
and identifies with ops.identify_pq (csrc/identify_pq.hip), which scores the decoded rows without ever storing them.
build(index="ivfpq"), compress() and load() make one; identify, identify_windows, timeline and match work on either
form; rows() and self_matches() need the flat one.

The half form keeps the rows as bf16 and their norms, nothing else: 260 bytes per row, a third of the flat form, with no
quantiser to train.  build(index="half"), halve(), from_half() and load() make one.  With U the f32 values of its bf16 rows
(exact), it answers identify, identify_windows, timeline, match and StreamMonitor bit for bit as the flat library over U
does: the search (ops.HalfL2Index) is exact over the rows held, ops.identify_half (csrc/identify_half.hip) and
ops.cross_match_half (csrc/crossmatch_half.hip) score them widened in registers.  Against the flat library over the f32
rows it was rounded from, a score moves by at most 2^-8 max||q|| max||x|| (HALF_SCORE_BOUND).  rows(), tempo=,
query_stride > 1, thin(), compress(), self_matches() and sharding need the flat form.

A flat library may keep only every D-th row of each track (build(row_stride=D), thin(D)): the catalogue is stored at
a coarse hop and the query stays dense, so some of its rows land exactly on kept rows whatever the true alignment is
and the offset is still resolved to one segment hop.  772 / D bytes per original row with exact f32 scores, a search
over D times fewer rows and a build that runs the model on D times fewer segments; identify, identify_windows and
timeline work on it through ops.identify_thin (csrc/identify_thin.hip).  compress(), self_matches() and match() need
every row (row_stride 1).

identify(tempo=...) and identify_windows(tempo=...) also find recordings that play a few per cent faster or slower
than the catalogue: the same embed and search, then one ops.identify_tempo launch (csrc/identify_tempo.hip) that scores
every candidate along the sloped alignment of each speed ratio of tempo_ratios(); timeline() follows such windows along
their slope.  match(tempo=...) does the same for whole recordings (one ops.cross_match_tempo launch per batch,
csrc/crossmatch_tempo.hip) and self_matches(tempo=...) for the tracks of the library itself (ops.self_match_tempo,
csrc/selfmatch_tempo.hip).  A flat library that keeps every row only; speed, not pitch.  StreamMonitor(tempo=...) follows live
channels the same way and, with tempo_lock, searches a channel whose speed has shown itself over three ratios only
(ops.identify_tempo_items, csrc/identify_tempo_items.hip: a ratio window per item).

identify(query_stride=Q) and identify_windows(query_stride=Q) are the query side's counterpart of row_stride: only the
segments 0, Q, 2 Q, ... of a recording are embedded and searched -- the encoder is nearly all of a query's cost -- and
one ops.identify_stride launch (csrc/identify_stride.hip) aligns them on the dense rows of the library; a query may
then hold 256 * Q segments.  A flat library that keeps every row only, no tempo; match() and self_matches() do not take
it; StreamMonitor does.

match() takes whole recordings of any length that are NOT in the library and says which tracks they share audio with,
where and how much (spans, coverage, votes: what self_matches says about the library's own tracks) -- the question an
ingest gate asks before add().  It runs on ops.cross_match (f32 rows) or ops.cross_match_pq (codes), the kernels of
csrc/crossmatch.hip, and with tempo=... on ops.cross_match_tempo (csrc/crossmatch_tempo.hip): a DJ set pitched a few
per cent or a sped-up re-upload is then one match along its sloped alignment, not fragments of diagonals.

A FingerprintLibrary lives on one device.  Its query calls (identify, identify_windows, timeline, match) are
LibraryFront's, written over the track table and three hooks: _search_rows, _identify_lists, _match_lists.
grafp_amd/sharded.py's ShardedFingerprintLibrary is the same front over several flat libraries of contiguous track
ranges, one per device, and answers with exactly what the one library over the same tracks would: every shard runs the
ops above unchanged (_identify_lists, _match_launch) and ops.merge_track_lists (csrc/merge_lists.hip) merges them on chip."""
import hashlib
import json
import math
import os

import numpy as np
import torch

from . import ops
from ._forms import FORMAT, FORMAT_COMPACT, FORMAT_HALF, FORMAT_THIN, FORMS, CompactForm, FlatForm, HalfForm

SETTINGS = ("fs", "n_fft", "win_len", "hop_len", "n_mels", "n_frames", "overlap")
# What the half form costs against the flat form over the f32 rows X it was rounded from.  bf16 keeps 8 significant bits,
# so round to nearest even moves a component by at most half an ulp, 2^-8 relative; then ||x^ - x|| <= 2^-8 ||x|| and
# (Cauchy-Schwarz) an inner product <q, x> moves by at most 2^-8 |q| |x|; a span score, a mean of such products, by at most
# HALF_SCORE_BOUND * max|q| * max|x|.  That is the worst case (every component at a tie, the error parallel to q); on real
# rows the errors are independent and the shift is a few 1e-5.
HALF_SCORE_BOUND = 2.0 ** -8
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


def kept_items(item_row, item_len, Q):
    """Items over the dense segments [item_row, item_row + item_len) of a recording, of which only the segments whose
    index is a multiple of Q are kept (kept row c is segment c * Q) -> (kept_row, kept_len), the same items over the kept
    rows: the first is c0 = ceil(item_row / Q), the count max(0, (item_row + item_len - 1) // Q - c0 + 1), 0 for an empty
    item.  An item with no kept row still gets c0 as its row."""
    j, n, Q = np.asarray(item_row, np.int64), np.asarray(item_len, np.int64), int(Q)
    c0 = -(-j // Q)
    cnt = np.where(n > 0, np.maximum(0, (j + n - 1) // Q - c0 + 1), 0)
    return c0.astype(np.int64), cnt.astype(np.int32)


def tempo_ratios(tempo, max_len, step=None):
    """The ratio grid of a tempo search over items of up to max_len segments, as ops.identify_tempo takes it: ascending
    int32 `num`, each standing for num / 256 track seconds per recording second.
    tempo: a float x in (0, 0.5] meaning the ratios [1 - x, 1 + x], or a pair (lo, hi) of ratios.  step: the grid's
    spacing in units of 1/256; by default g = max(1, 256 // max_len), with which the nearest grid ratio is at most half
    a row off at the item's end.  The result is 256 + i * g for the integers i that land inside
    [ceil(256 * lo), floor(256 * hi)] clipped to [128, 512]."""
    if isinstance(tempo, (tuple, list, np.ndarray)):
        if len(tempo) != 2:
            raise ValueError(f"tempo must be one number or a pair (lo, hi) of ratios, got {tempo!r}")
        lo, hi = float(tempo[0]), float(tempo[1])
    else:
        x = float(tempo)
        if not 0.0 < x <= 0.5:
            raise ValueError(f"tempo={x} must lie in (0, 0.5]: the ratios searched are [1 - tempo, 1 + tempo]")
        lo, hi = 1.0 - x, 1.0 + x
    if not lo <= hi:
        raise ValueError(f"tempo=({lo}, {hi}): the lower ratio is above the upper one")
    g = max(1, ops.IDENTIFY_TEMPO_DEN // max(1, int(max_len))) if step is None else int(step)
    if g < 1:
        raise ValueError(f"tempo: step={g} must be at least 1 (in units of 1/256)")
    a = max(ops.IDENTIFY_TEMPO_MIN, int(math.ceil(ops.IDENTIFY_TEMPO_DEN * lo - 1e-9)))
    b = min(ops.IDENTIFY_TEMPO_MAX, int(math.floor(ops.IDENTIFY_TEMPO_DEN * hi + 1e-9)))
    i0, i1 = -((ops.IDENTIFY_TEMPO_DEN - a) // g), (b - ops.IDENTIFY_TEMPO_DEN) // g
    nums = ops.IDENTIFY_TEMPO_DEN + g * np.arange(i0, i1 + 1, dtype=np.int64)
    if nums.size == 0:
        raise ValueError(f"tempo: no ratio 256 + i * {g} lies in [{a}, {b}] / 256; give a smaller step")
    if nums.size > ops.IDENTIFY_TEMPO_MAX_RATIOS:
        raise ValueError(f"tempo: {nums.size} ratios from {a} to {b} at step={g} exceed the "
                         f"{ops.IDENTIFY_TEMPO_MAX_RATIOS} of one launch; give a larger step or a narrower range")
    return nums.astype(np.int32)


def tempo_span(lo, m, num):
    """The other side of a span of m rows from row lo on at ratio num / 256, where row i sits w(i) = (i * num + 128) >> 8
    rows after the other side's reference row: -> (w(lo), w(lo + m - 1) - w(lo) + 1), its first row and its rows.  At
    num = 256: (lo, m)."""
    half = ops.IDENTIFY_TEMPO_DEN // 2
    w_lo, w_hi = (lo * num + half) >> 8, ((lo + m - 1) * num + half) >> 8
    return w_lo, w_hi - w_lo + 1


def track_table(counts):
    """Row counts per track, in order -> the int64 track table: track t owns rows [first[t], first[t+1])."""
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def track_names(names, n_tracks, base=0):
    """The names of n_tracks new tracks behind `base` existing ones: str() of the given ones, or track{base + i}."""
    names = [str(v) for v in names] if names is not None else [f"track{base + i}" for i in range(n_tracks)]
    if len(names) != n_tracks:
        raise ValueError(f"{len(names)} names for {n_tracks} tracks")
    return names


def batch_ranges(counts, limit):
    """The batching rule of self_matches and match over items of counts[i] rows: a batch of consecutive items closes
    once it holds at least `limit` rows (limit <= 0: every item alone), the last takes the rest.  -> ranges (i0, i1)."""
    out, i0, held = [], 0, 0
    for i, n in enumerate(counts):
        held += int(n)
        if held >= limit or i == len(counts) - 1:
            out.append((i0, i + 1))
            i0, held = i + 1, 0
    return out


def span_slots(res, sources, has_ratio, min_score, what):
    """The walk over the outputs of a span op (ops.self_match, ops.cross_match, their kin): res = (partner, delta, start,
    length, score, votes[, ratio]), each (len(sources), top), read back here.  Yields (source, partner, ..., votes, ratio
    or None) per filled slot: a negative partner ends a source, a score under min_score is skipped, the -2 mark raises."""
    cols = [x.cpu().numpy() for x in res[:7 if has_ratio else 6]]
    for s, src in enumerate(sources):
        for j in range(cols[0].shape[1]):
            b = int(cols[0][s, j])
            if b == -2:                                              # the op sizes the workspace exactly: never
                raise RuntimeError(f"{what} {src} did not fit the workspace")
            if b < 0:
                break
            sc = float(cols[4][s, j])
            if min_score is not None and sc < min_score:
                continue
            yield (src, b, int(cols[1][s, j]), int(cols[2][s, j]), int(cols[3][s, j]), sc, int(cols[5][s, j]),
                   int(cols[6][s, j]) if has_ratio else None)


def is_single(queries):
    """Whether identify and match were given one query (a path or a 1-D waveform) and answer with its list alone."""
    return isinstance(queries, str) or (isinstance(queries, (np.ndarray, torch.Tensor)) and
                                        torch.as_tensor(queries).dim() == 1)


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


class LibraryFront:
    """The query front of a fingerprint library: the sizes, the refusals, fingerprinting and identify, identify_windows,
    timeline and match, written once over the shared state -- model, settings, precision, device (where the model runs
    and the queries are embedded), first, names and _row_stride.  A library (FingerprintLibrary,
    sharded.ShardedFingerprintLibrary) derives from it and implements is_compact and the three hooks _search_rows,
    _identify_lists and _match_lists: the interface that StreamMonitor, the sharded library and the tools rely on."""

    def __init__(self, model, settings, precision, device, row_stride):
        self.model, self.device, self.precision, self._row_stride = model, device, precision, int(row_stride)
        self.settings = {k: settings[k] for k in SETTINGS}
        self.first, self.names = np.zeros(1, np.int64), []

    # ---- what a library implements ----------------------------------------------------------------------------
    @property
    def is_compact(self):
        """Whether the library holds IVF-PQ codes and no f32 rows."""
        raise NotImplementedError

    @property
    def is_half(self):
        """Whether the library holds bf16 rows and no f32 rows (a FingerprintLibrary made by build(index="half"),
        halve(), from_half() or load())."""
        return False

    def _search_rows(self, q, k_probe):
        """q (n, 128) f32 -> ids (n, min(k_probe, n_rows)) int64, each row's nearest library rows, on the device."""
        raise NotImplementedError

    def _identify_lists(self, q, ids, item_row, item_len, top, min_overlap, max_len, nums=None, q_stride=1,
                        item_ratios=None):
        """The launch of _identify_items -> the op's device tensors (track, offset, score, votes and, with the ratio
        grid nums, ratio), nothing read back.  q_stride: the items' rows are every q_stride-th segment of the
        recording (min_overlap and max_len then count those rows).  item_ratios: None, or with nums the pair of host
        arrays (lo, cnt) of ops.identify_tempo_items: item i is searched over nums[lo_i : lo_i + cnt_i] only.  (The
        front passes the keyword only when it is set.)"""
        raise NotImplementedError

    def _match_lists(self, qb, src, k_probe, nums, kw):
        """The search and the launch of one batch of _match_rows: qb the batch's rows, src its source table (a host
        tensor) -> the op's device tensors (track, delta, start, length, score, votes and, with nums, ratio), nothing
        read back."""
        raise NotImplementedError

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

    @property
    def row_stride(self):
        """D: row j of a track is the track's segment j * D (a dense library: 1).  Offsets stay in segments."""
        return self._row_stride

    def _need_dense(self, what):
        if self._row_stride != 1:
            raise NotImplementedError(f"FingerprintLibrary.{what} needs every row of a track: this library keeps every "
                                      f"{self._row_stride}th (row_stride={self._row_stride})")

    def _need_flat(self, what, instead="build(index='flat') keeps the f32 rows that it needs"):
        if self.is_half:
            raise NotImplementedError(f"FingerprintLibrary.{what} is not built for the half form of a library (bf16 rows "
                                      f"only): {instead}")
        if self.is_compact:
            raise NotImplementedError(f"FingerprintLibrary.{what} needs the flat form of a library (f32 rows): this one "
                                      "is compact and holds IVF-PQ codes only")

    def _need_tempo_form(self, what, tempo):
        if tempo is not None:
            self._need_flat(f"{what}(tempo=...)")
            self._need_dense(f"{what}(tempo=...)")

    def _need_stride_form(self, what, query_stride, tempo=None):
        """The checks of a query_stride: an integer in [1, ops.IDENTIFY_MAX_QUERY_STRIDE]; above 1 it needs a flat
        library that keeps every row, and no tempo.  -> the stride as an int."""
        Q = int(query_stride)
        if Q != query_stride or not 1 <= Q <= ops.IDENTIFY_MAX_QUERY_STRIDE:
            raise ValueError(f"query_stride={query_stride} not in [1, {ops.IDENTIFY_MAX_QUERY_STRIDE}]")
        if Q > 1:
            if tempo is not None:
                raise NotImplementedError(f"FingerprintLibrary.{what}(query_stride={Q}) with tempo=... is not built: "
                                          "a strided query is identified at the catalogue's speed only")
            self._need_flat(f"{what}(query_stride={Q})")
            self._need_dense(f"{what}(query_stride={Q})")
        return Q

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

    def _fingerprint_batches(self, waves, max_segments, counts):
        """Segments of consecutive tracks packed into model calls as fpdb._embed_stream packs them in eval mode (a call
        once at least max_segments segments are pending): yields the rows of one call after the other and appends every
        track's row count to `counts`."""
        pend, n_pend = [], 0
        for w in waves:
            segs = self.segments(w)[::self._row_stride]              # (a thinned library embeds the kept segments only)
            counts.append(segs.shape[0])
            pend.append(segs)
            n_pend += segs.shape[0]
            if n_pend >= max_segments:
                yield self._embed(torch.cat(pend, dim=0))
                pend, n_pend = [], 0
        if n_pend:
            yield self._embed(torch.cat(pend, dim=0))

    def _fingerprint_tracks(self, waves, max_segments):
        """-> (rows, per-track row counts) of _fingerprint_batches."""
        counts = []
        out = list(self._fingerprint_batches(waves, max_segments, counts))
        rows = torch.cat(out, dim=0) if out else torch.zeros((0, 128), device=self.device)
        return rows, counts

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

    def _check_item_len(self, max_len, k_probe):
        if max_len > ops.IDENTIFY_MAX_LEN or max_len * k_probe > ops.IDENTIFY_MAX_KEYS:
            raise ValueError(f"a query of {max_len} segments ({max_len * self.segment_s:.1f} s) with k_probe={k_probe} "
                             f"exceeds {ops.IDENTIFY_MAX_LEN} segments / {ops.IDENTIFY_MAX_KEYS} hits per item: use "
                             "identify_windows for long recordings")

    def _embed_and_search(self, segs, k_probe):
        """One batched embed of the segments and one search of their rows -> (q (n, 128) f32, ids (n, k) int64)."""
        q = self._embed(segs)
        return q, self._search_rows(q, k_probe)

    def _identify_items(self, q, ids, item_row, item_len, top, min_overlap, max_len=None, tempo=None, tempo_step=None,
                        q_stride=1, ratio_window=None):
        """One identify launch (the kernel of the library's form) for all items over the rows q and their hits ids ->
        per-item lists of matches.  max_len: an upper bound of the items' lengths (None: the longest).  (StreamMonitor
        calls it with rows it kept from earlier pushes.)  tempo: tempo_ratios' argument; the launch is then
        ops.identify_tempo over the ratio grid of the longest item, and every match names its ratio.  q_stride: the rows
        q are every q_stride-th segment of the recording and the items count those rows; min_overlap stays in dense
        segments (the op gets max(1, min_overlap // q_stride) pairs) and the offsets in dense segments.
        ratio_window: None, or with tempo a pair of arrays (lo, cnt), one value per item, of indices into the ratio
        grid derived here: item i is searched over grid[lo_i : lo_i + cnt_i] only (ops.identify_tempo_items; the tempo
        lock of StreamMonitor, which fixes the grid by giving tempo_step)."""
        n_items = len(item_row)
        longest = int(np.max(item_len, initial=0))
        if n_items == 0 or longest == 0:
            return [[] for _ in range(n_items)]
        max_len = longest if max_len is None else max(int(max_len), longest)
        nums = None if tempo is None else tempo_ratios(tempo, longest, tempo_step)
        if q_stride != 1 and min_overlap is not None:
            min_overlap = max(1, int(min_overlap) // q_stride)
        kw = {}
        if ratio_window is not None:
            if nums is None:
                raise ValueError("ratio_window needs tempo: it indexes the tempo search's ratio grid")
            kw["item_ratios"] = (np.asarray(ratio_window[0], np.int64), np.asarray(ratio_window[1], np.int64))
        lists = self._identify_lists(q, ids, np.asarray(item_row, np.int64), np.asarray(item_len, np.int32), top,
                                     min_overlap, max_len, nums, q_stride, **kw)
        tr, off, sc, vo = (t.cpu().numpy() for t in lists[:4])
        ra = lists[4].cpu().numpy() if nums is not None else None
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
                if ra is not None:
                    res[-1]["tempo"] = int(ra[i, j]) / ops.IDENTIFY_TEMPO_DEN
                    res[-1]["tempo_num"] = int(ra[i, j])
            out.append(res)
        return out

    def _search_and_identify(self, segs, item_row, item_len, top, k_probe, min_overlap, tempo=None, tempo_step=None,
                             q_stride=1):
        """One batched embed + search of all segments, one ops.identify launch for all items -> per-item lists.  (The
        segments given are all embedded, whatever the library's row_stride: against a thinned library the query side
        stays dense.  q_stride: segs are every q_stride-th segment of the recordings and the items count those.)"""
        n_items = len(item_row)
        if tempo is not None:
            tempo_ratios(tempo, max(1, int(np.max(item_len, initial=0))), tempo_step)      # refuse a bad range early
        if n_items == 0 or segs.shape[0] == 0 or self.n_rows == 0 or int(np.max(item_len, initial=0)) == 0:
            return [[] for _ in range(n_items)]
        self._check_item_len(int(np.max(item_len)), k_probe)
        q, ids = self._embed_and_search(segs, k_probe)
        return self._identify_items(q, ids, item_row, item_len, top, min_overlap, tempo=tempo, tempo_step=tempo_step,
                                    q_stride=q_stride)

    def identify(self, queries, fs=None, top=5, k_probe=20, min_overlap=None, tempo=None, tempo_step=None,
                 query_stride=1):
        """queries: one waveform, a list of ragged waveforms, or file paths; at `fs` (default settings['fs']; other rates
        are resampled on the device).  -> per query, a list of matches {track, name, offset, offset_s, score, votes},
        best first.  offset_s = offset * step * hop_len / fs is where the query's first segment sits in the track.  A
        query shorter than one segment gives an empty list.
        tempo: None, or the speeds to search for a recording that plays faster or slower than the catalogue -- a float
        x in (0, 0.5] for the ratios [1 - x, 1 + x] (track seconds per recording second), or a pair (lo, hi);
        tempo_step: the ratio grid's spacing in 1/256 (tempo_ratios; default: from the longest query).  The segments
        are embedded and searched as without it and one ops.identify_tempo launch scores every candidate along the
        sloped alignment of every ratio; each match then also carries "tempo" (the ratio) and "tempo_num" (ratio *
        256), and offset / offset_s keep their meaning.  Needs a flat library that keeps every row.  Speed only: pitch
        is not searched; match() takes the same tempo for whole recordings and self_matches() for the tracks of the
        library itself and StreamMonitor for live channels; the IVF-PQ and the thinned forms know no tempo.
        query_stride: Q in [1, 32]; above 1 only the segments 0, Q, 2 Q, ... of every query are embedded and searched
        (1 / Q of the model's work) and one ops.identify_stride launch aligns them (csrc/identify_stride.hip).  The
        matches keep their form and offset / offset_s their meaning; min_overlap stays in dense segments (the kernel
        asks for max(1, min_overlap // Q) pairs); a query may then hold 256 * Q segments.  Needs a flat library that
        keeps every row, and no tempo."""
        self._need_tempo_form("identify", tempo)
        Q = self._need_stride_form("identify", query_stride, tempo)
        single = is_single(queries)
        waves = self._load_queries(queries, fs)
        segs = [self.segments(w)[::Q] for w in waves]
        lens = np.array([s.shape[0] for s in segs], np.int32)
        allsegs = torch.cat(segs, dim=0) if segs else torch.empty((0,), device=self.device)
        res = self._search_and_identify(allsegs, track_table(lens)[:-1], lens, int(top), int(k_probe), min_overlap,
                                        tempo, tempo_step, Q)
        return res[0] if single and len(res) == 1 else res

    def identify_windows(self, recording, window_s=3.0, hop_s=1.0, fs=None, top=5, k_probe=20, min_overlap=None,
                         tempo=None, tempo_step=None, query_stride=1):
        """A long recording cut into items of window_s seconds every hop_s seconds.  The recording is segmented,
        fingerprinted and searched once; all windows are identified in one launch.  -> per window
        {start_s, end_s, segment_start_s, matches}; segment_start_s is where the window's first segment starts in the
        recording (the time its matches' offset_s refers to).  tempo, tempo_step: as for identify().
        query_stride: as for identify(); the recording's segments 0, Q, 2 Q, ... are embedded once, the windows stay
        those of window_items and each takes the kept segments inside it (kept_items), so segment_start_s is a multiple
        of Q segment hops; a window that holds no kept segment keeps the dense segment_start_s and has no matches."""
        self._need_tempo_form("identify_windows", tempo)
        Q = self._need_stride_form("identify_windows", query_stride, tempo)
        wave = self._load_queries([recording], fs)[0]
        segs = self.segments(wave)
        starts, rows, lens = window_items(segs.shape[0], wave.numel(), self.settings, window_s, hop_s)
        first_seg = rows
        if Q > 1:
            segs = segs[::Q].contiguous()
            rows, lens = kept_items(rows, lens, Q)
            first_seg = np.where(lens > 0, rows * Q, first_seg)
        res = self._search_and_identify(segs, rows, lens, int(top), int(k_probe), min_overlap, tempo, tempo_step, Q)
        seg_s = self.segment_s
        return [{"start_s": float(s), "end_s": float(s) + window_s, "segment_start_s": int(r) * seg_s, "matches": m}
                for s, r, m in zip(starts, first_seg, res)]

    def timeline(self, windows, min_score=None):
        """What played when: consecutive windows whose best match is the same track at a consistent position (the
        track offset minus the window's segment start agrees within one segment hop) merge into one span.
        -> list of {start_s, end_s, track, name, track_offset_s (the track position at start_s), score (mean)}.
        A window whose match carries a "tempo" rho (identify_windows(tempo=...)) is followed along its slope: the span
        keeps its last merged window (u = segment_start_s, o = offset_s, rho), and the next window (u', o') of the same
        track merges iff |o' - (o + rho * (u' - u))| is within one segment hop and it starts no later than the span's
        end; the reference point then advances.  Such a span also reports "tempo", the mean of its windows' rho."""
        spans, seg_s = [], self.segment_s
        for w in windows:
            if not w["matches"] or (min_score is not None and w["matches"][0]["score"] < min_score):
                continue
            m = w["matches"][0]
            if "tempo" in m:
                u, o, rho = w["segment_start_s"], m["offset_s"], m["tempo"]
                last = spans[-1] if spans else None
                if (last is not None and last["track"] == m["track"] and "_ref" in last
                        and abs(o - (last["_ref"][1] + last["_ref"][2] * (u - last["_ref"][0]))) <= seg_s + 1e-9
                        and w["start_s"] <= last["end_s"]):
                    last["end_s"] = w["end_s"]
                    last["_scores"].append(m["score"])
                    last["_tempos"].append(rho)
                else:
                    spans.append({"start_s": w["start_s"], "end_s": w["end_s"], "track": m["track"], "name": m["name"],
                                  "track_offset_s": o + rho * (w["start_s"] - u), "_scores": [m["score"]],
                                  "_tempos": [rho]})
                spans[-1]["_ref"] = (u, o, rho)
                continue
            delta = m["offset_s"] - w["segment_start_s"]              # track time = recording time + delta
            last = spans[-1] if spans else None
            if (last is not None and last["track"] == m["track"] and "_delta" in last
                    and abs(delta - last["_delta"]) <= seg_s + 1e-9
                    and w["start_s"] <= last["end_s"]):
                last["end_s"] = w["end_s"]
                last["_scores"].append(m["score"])
            else:
                spans.append({"start_s": w["start_s"], "end_s": w["end_s"], "track": m["track"], "name": m["name"],
                              "track_offset_s": w["start_s"] + delta, "_delta": delta, "_scores": [m["score"]]})
        for s in spans:
            s["score"] = float(np.mean(s.pop("_scores")))
            s.pop("_delta", None)
            if s.pop("_ref", None) is not None:
                s["tempo"] = float(np.mean(s.pop("_tempos")))
        return spans

    # ---- recordings against the catalog -------------------------------------------------------------------------
    def match(self, recordings, fs=None, k_probe=20, min_overlap_s=3.0, min_votes=4, min_score=None, top=8,
              max_segments=4096, batch_rows=1 << 18, tempo=None, tempo_step=None):
        """What whole recordings share with the library: is an upload already in the catalogue, in whole or in part,
        which tracks does a mix or medley contain, and where.  recordings: as identify's queries (one waveform, a list
        of ragged waveforms, or file paths, at `fs`; other rates are resampled on the device), of any length.  They are
        segmented, embedded in model calls of at least max_segments segments, searched with self.index (k_probe hits per
        row) and matched in launches of about batch_rows rows by ops.cross_match (flat) or ops.cross_match_pq (compact);
        nothing is added to the library.
        -> per recording, a list of {track, name, score, votes, offset, recording_start_s, track_start_s, overlap_s,
        coverage, recording_coverage, track_coverage}, best first (a single recording: its list alone, as identify).  The
        recording's audio from recording_start_s reappears in `track` from track_start_s for overlap_s seconds; offset =
        delta in segments (row i of the recording sits on row i + offset of the track); coverage = overlapping rows /
        rows of the shorter of the two, recording_coverage and track_coverage the same over the rows of each; score =
        mean cosine over the span; votes = rows whose hits agree on the alignment.  At most `top` tracks per recording,
        each at its best alignment.  min_overlap_s, min_votes and min_score as for self_matches.  A recording shorter
        than one segment, or an empty library, gives [].
        k_probe = 20 is identify's default; it has not been measured for this use (self_matches uses 32 because it
        drops a row's hits on its own track; nothing is dropped here).
        One recording is one workgroup, as a track is in self_matches: an hour-long recording is not split into pieces,
        its hits are sorted through the launch's workspace (ops.self_match_workspace_bytes of the batch's row counts).
        tempo: None, or the speeds to search, as identify takes them (a float x for the ratios [1 - x, 1 + x] of track
        seconds per recording second, or a pair (lo, hi)); tempo_step: the ratio grid's spacing in 1/256, by default 1
        (recordings are long: at a coarser grid the nearest ratio drifts off a long span).  The launches then go to
        ops.cross_match_tempo, R ratios at once, in batches of about batch_rows // R rows (the workspace is R times a
        dense launch's), and row i of the recording sits on row offset + w(i) of the track, w(i) = (i * tempo_num + 128)
        >> 8.  Each match also carries tempo (= tempo_num / 256), tempo_num and track_overlap_s = (w(i_hi) - w(i_lo) +
        1) segment hops, the track's side of the span; track_start_s = (offset + w(i_lo)) hops, recording_coverage = m /
        recording rows, track_coverage = (w(i_hi) - w(i_lo) + 1) / track rows, coverage the larger of the two (at 256:
        the dense m / min).  When the true ratio lies between two grid ratios a long span drifts off its alignment by
        up to a row per 512 rows and may end early: overlap_s is then a lower bound of the shared audio.  Needs a flat
        library that keeps every row."""
        self._need_tempo_form("match", tempo)
        self._need_dense("match()")
        nums = None if tempo is None else tempo_ratios(tempo, ops.IDENTIFY_TEMPO_DEN, tempo_step)   # step 1 by default
        single = is_single(recordings)
        waves = self._load_queries(recordings, fs)
        if self.n_rows == 0:
            res = [[] for _ in waves]
        else:
            rows, counts = self._fingerprint_tracks(waves, int(max_segments))
            res = self._match_rows(rows, counts, int(k_probe), float(min_overlap_s), int(min_votes), min_score,
                                   int(top), int(batch_rows), nums)
        return res[0] if single and len(res) == 1 else res

    def _match_entry(self, b, d, lo, m, sc, v, n_rec, num=None):
        """One match of match() from one slot of the kernel's outputs: partner b, delta d, span start lo, span rows m,
        score, votes, for a recording of n_rec rows; num: the winning ratio of ops.cross_match_tempo (None: dense)."""
        seg_s = self.segment_s
        lr, lt = max(1, int(n_rec)), max(1, int(self.first[b + 1] - self.first[b]))
        w_lo, mt = (lo, m) if num is None else tempo_span(lo, m, num)     # the track's side of the span (dense: the same)
        entry = {"track": b, "name": self.names[b], "score": sc, "votes": v,
                 "offset": d, "recording_start_s": lo * seg_s, "track_start_s": (d + w_lo) * seg_s,
                 "overlap_s": m * seg_s, "coverage": max(m / lr, mt / lt),
                 "recording_coverage": m / lr, "track_coverage": mt / lt}
        if num is not None:
            entry.update({"tempo": num / ops.IDENTIFY_TEMPO_DEN, "tempo_num": num, "track_overlap_s": mt * seg_s})
        return entry

    def _match_rows(self, q, counts, k_probe, min_overlap_s, min_votes, min_score, top, batch_rows, nums=None):
        """match() from the recordings' rows on: q (n_q, 128) f32 on the device, counts the rows of each recording.
        nums: the ratio grid of match(tempo=...) (None: the dense kernels)."""
        min_overlap = max(1, int(math.ceil(min_overlap_s / self.segment_s - 1e-9)))
        starts = track_table(counts)
        out = [[] for _ in counts]
        if nums is not None:
            batch_rows = batch_rows // len(nums)                     # the workspace is R times a dense launch's
        for s0, s1 in batch_ranges(counts, batch_rows):
            qb = q[int(starts[s0]):int(starts[s1])]
            if qb.shape[0]:
                res = self._match_lists(qb, torch.from_numpy(starts[s0:s1 + 1] - starts[s0]), k_probe, nums,
                                        dict(top=top, min_votes=min_votes, min_overlap=min_overlap))
                for s, b, d, lo, m, sc, v, num in span_slots(res, range(s0, s1), nums is not None, min_score,
                                                             "cross_match: recording"):
                    out[s].append(self._match_entry(b, d, lo, m, sc, v, counts[s], num))
        return out


class FingerprintLibrary(LibraryFront):
    """Fingerprints of whole tracks, resident on one device, with the table that says which rows are which track."""

    def __init__(self, model, settings, rows, first, names=None, precision="bf16", device=None, row_stride=1):
        if precision not in ("bf16", "f32"):
            raise ValueError(f"precision must be 'bf16' or 'f32', not {precision!r}")
        if not 1 <= int(row_stride) <= ops.IDENTIFY_MAX_STRIDE:
            raise ValueError(f"row_stride={row_stride} not in [1, {ops.IDENTIFY_MAX_STRIDE}]")
        super().__init__(model, settings, precision,
                         torch.device(device) if device is not None else next(model.parameters()).device, row_stride)
        # the rows: chunks of the form's tuple of tensors ((rows,), or (list_id, codes)), as they were appended
        self._chunks, self._held, self._index = [], None, None
        self._form = FlatForm(self.device, row_stride)               # how they are held (_forms.py): flat, half or compact
        if rows is not None:
            self._append(rows, first, names)

    @classmethod
    def from_codes(cls, model, settings, quantiser, list_id, codes, first, names=None, precision="bf16", device=None,
                   nprobe=20):
        """A compact library over rows that are already encoded: quantiser {"centroids" (nlist, 128), "codebooks"
        (M, 256, 128 // M)}, list_id (n) and codes (n, M) uint8 in row order, the track table as for the constructor.
        Works on device="cpu" (files and tables only), like the flat form."""
        lib = cls(model, settings, None, None, precision=precision, device=device)
        lib._set_quantiser(quantiser, nprobe)
        lib._append_codes(list_id, codes, first, names)
        return lib

    @classmethod
    def from_half(cls, model, settings, rows_bf16, first, names=None, precision="bf16", device=None):
        """A half library over rows that are already bf16: rows_bf16 (n, 128) torch.bfloat16, or their bit patterns as
        uint16 (a numpy array, what save() writes); the track table as for the constructor.  With U the rows' f32 values
        it answers every call it supports bit for bit as the flat library over U does.  Works on device="cpu" (files and
        tables only), like from_codes."""
        lib = cls(model, settings, None, None, precision=precision, device=device)
        lib._form = HalfForm(lib.device)
        lib._append_half(rows_bf16, first, names)
        return lib

    def _set_quantiser(self, quantiser, nprobe):
        self._form, self._held = CompactForm(self.device, quantiser, nprobe), None

    @property
    def is_compact(self):
        return self._form.is_compact

    @property
    def is_half(self):
        return self._form.is_half

    def _need_half(self, what):
        if not self.is_half:
            raise ValueError(f"FingerprintLibrary.{what}: {HalfForm.missing}")

    def half_rows(self):
        """The resident (n_rows, 128) bf16 fingerprints of a half library: the tensor its index searches."""
        self._need_half("half_rows()")
        return self._stored()[0]

    def quantiser(self):
        """{"centroids", "codebooks"} of a compact library (device tensors)."""
        self._need_compact("quantiser()")
        return self._form.quantiser()

    def _need_compact(self, what):
        if not self.is_compact:
            raise ValueError(f"FingerprintLibrary.{what}: {CompactForm.missing}")

    @property
    def nbytes(self):
        """Device bytes the library holds: its rows (flat) or its row-order codes, list ids and quantiser (compact),
        plus its index, which is made here if the device has one (on a CPU device only the library's own tensors count).
        Flat: 772 bytes per row.  Compact: 2 M + 20 per row, plus the quantiser and the index's two nlist-sized tables.
        Half: 260 bytes per row -- the bf16 rows, which the index shares, and its norms."""
        held = self._form.held_tensors(self._stored())
        if self.device.type == "cuda" and self.n_rows:
            held += self.index.held_tensors()
        seen = {t.untyped_storage().data_ptr(): t.untyped_storage().nbytes() for t in held}
        return int(sum(seen.values()))

    def _stored(self):
        """All rows as one tuple of tensors, (rows,) (f32, or bf16 in the half form) or (list_id, codes): the chunks
        concatenated on first use and kept as the one chunk; a library without rows gives its form's empty tensors."""
        if self._held is None:
            if len(self._chunks) > 1:
                self._chunks = [tuple(torch.cat(part) for part in zip(*self._chunks))]
            self._held = self._chunks[0] if self._chunks else self._form.empty()
        return self._held

    def rows(self):
        """The resident (n_rows, 128) f32 fingerprints (flat form only)."""
        self._need_flat("rows()", "half_rows() gives its bf16 rows, half_rows().float() their exact f32 values")
        return self._stored()[0]

    def codes(self):
        """(list_id (n_rows) int32, codes (n_rows, M) uint8) of a compact library, in row order."""
        self._need_compact("codes()")
        return self._stored()

    @property
    def index(self):
        """The index over the rows, made on first use: the ops.FlatL2Index over rows() (it shares the rows tensor), or,
        for a compact library, the ivfpq.IVFPQIndex over codes() (from_codes: nothing is re-encoded, the row-order codes
        are shared), or, for a half library, the ops.HalfL2Index over half_rows() (it shares that tensor)."""
        if self._index is None:
            self._index = self._form.index(self._stored())
        return self._index

    def _store(self, n_new, chunk, first, names):
        """The tail of _append and _append_codes: n_new rows of new tracks with their own table `first` go behind the
        library's.  chunk() -> their tuple of device tensors, asked for only if there are rows."""
        first = np.asarray(first, np.int64).reshape(-1)
        ops.check_track_table(first, n_new)
        names = track_names(names, len(first) - 1, self.n_tracks)
        if n_new:
            self._chunks.append(chunk())
            self._held, self._index = None, None
        self.first = np.concatenate([self.first, self.first[-1] + first[1:]])
        self.names += names

    def _append(self, rows, first, names):
        self._need_flat("_append()")
        self._store(*self._form.chunk(rows), first, names)

    def _append_half(self, rows_bf16, first, names):
        self._need_half("_append_half()")
        self._store(*self._form.chunk(rows_bf16), first, names)

    def _append_codes(self, list_id, codes, first, names):
        self._need_compact("_append_codes()")
        self._store(*self._form.chunk(list_id, codes), first, names)

    def _fingerprint_codes(self, waves, max_segments, train):
        """build(index="ivfpq") without a quantiser: fingerprint and encode one model call after the other; the f32 rows
        of a call are dropped once encoded.  train = (nlist, pq_m, nprobe, train_rows, seed): the rows of the first
        calls are held until train_rows of them are there (or the input ends), the quantiser is trained on them (the
        library is compact from then on), they are encoded, and every later call is encoded as it comes -- never more f32
        rows alive than train_rows plus one call's (max_segments, rounded up to whole tracks).  -> (list_id, codes,
        per-track row counts)."""
        counts, held, n_held, out = [], [], 0, []
        for rows in self._fingerprint_batches(waves, max_segments, counts):
            if held is not None:
                held.append(rows)
                n_held += rows.shape[0]
                if n_held < train[3]:
                    continue
                rows, held = torch.cat(held), None
                self._train_quantiser(rows, *train[:3], rows.shape[0], train[4])
            if rows.shape[0]:
                out.append(self._form.encode(rows))
        if held is not None:                                 # the input ended before train_rows rows were there
            if n_held == 0:
                raise ValueError("an IVF-PQ library cannot be trained on tracks that give no fingerprint rows")
            rows = torch.cat(held)
            self._train_quantiser(rows, *train[:3], rows.shape[0], train[4])
            out.append(self._form.encode(rows))
        data = tuple(torch.cat(part) for part in zip(*out)) if out else self._form.empty()
        return (*data, counts)

    def _train_quantiser(self, rows, nlist, pq_m, nprobe, train_rows, seed):
        """Both k-means of ivfpq.IVFPQIndex.train on `rows` (at most train_rows of them, a seeded sample in row order)."""
        from .ivfpq import IVFPQIndex
        if int(pq_m) not in ops.IDENTIFY_PQ_M:
            raise ValueError(f"pq_m={pq_m} not one of {ops.IDENTIFY_PQ_M}")
        if rows.shape[0] > int(train_rows):
            gen = torch.Generator().manual_seed(int(seed) + 1)
            sel = torch.sort(torch.randperm(rows.shape[0], generator=gen)[:int(train_rows)]).values
            rows = rows[sel.to(rows.device)]
        trainer = IVFPQIndex(d=128, nlist=int(nlist), M=int(pq_m), device=self.device, seed=int(seed), keep_raw=False)
        trainer.train(rows)
        self._set_quantiser(trainer.quantiser(), nprobe)

    @classmethod
    def build(cls, model, tracks, cfg, names=None, precision="bf16", max_segments=4096, index="flat", nlist=64, pq_m=64,
              nprobe=20, train_rows=65536, quantiser=None, seed=1234, row_stride=1):
        """Fingerprint whole tracks (a DeviceAudioCorpus, its .tracks(), or 1-D tensors / arrays at cfg['fs']) into a
        new library.  Tracks shorter than one segment get no rows: they stay in the table and never match.
        index="ivfpq": a compact library.  Its quantiser (nlist lists, pq_m sub-quantisers) is trained on the rows of
        the first model calls, as soon as they hold train_rows rows (on all rows if there are fewer); every later
        model call is encoded and its f32 rows dropped, so the f32 rows of the catalogue never exist at once.
        quantiser={"centroids", "codebooks"}: nothing is trained.
        index="half": a half library, the bf16 rows and their norms only (260 bytes a row against the flat form's 772).
        Every model call's rows are rounded to bf16 (round to nearest even) as they come and the f32 rows dropped, so the
        f32 rows of the catalogue never exist at once; nothing is trained.  The search stays exact over the rows held.
        row_stride=D (flat only): every D-th segment of each track is fingerprinted and kept, selected before the model
        call -- 1 / D of the model work and of the rows; a track of S segments gets ceil(S / D) rows."""
        if index not in ("flat", "ivfpq", "half"):
            raise ValueError(f"index must be 'flat', 'ivfpq' or 'half', not {index!r}")
        if index == "half":
            if int(row_stride) != 1:
                raise NotImplementedError(f"build(index='half') needs every row of a track: a thinned half library "
                                          f"(row_stride={row_stride}) is not built; use index='flat' with row_stride")
            lib = cls(model, cfg, None, None, precision=precision)
            lib._form = HalfForm(lib.device)
            return lib.add(tracks, names=names, max_segments=max_segments)
        if index == "ivfpq" and int(row_stride) != 1:
            raise NotImplementedError(f"build(index='ivfpq') needs every row of a track: row_stride={row_stride} codes "
                                      "are not implemented")
        lib = cls(model, cfg, None, None, precision=precision, row_stride=row_stride)
        if index == "flat":
            return lib.add(tracks, names=names, max_segments=max_segments)
        if quantiser is not None:
            lib._set_quantiser(quantiser, nprobe)
            return lib.add(tracks, names=names, max_segments=max_segments)
        waves, own = _as_waveforms(tracks)
        a, codes, counts = lib._fingerprint_codes(waves, int(max_segments), (nlist, pq_m, nprobe, train_rows, seed))
        lib._append_codes(a, codes, track_table(counts), names if names is not None else own)
        return lib

    def add(self, tracks, names=None, max_segments=4096):
        """Append tracks (as for build) to the library; a compact library encodes them with its own quantiser, a
        thinned one keeps every row_stride-th segment of each, a half one rounds each model call's rows to bf16."""
        waves, own = _as_waveforms(tracks)
        counts = []
        parts = [self._form.encode(rows) for rows in self._fingerprint_batches(waves, int(max_segments), counts)
                 if rows.shape[0]]
        data = tuple(torch.cat(part) for part in zip(*parts)) if parts else self._form.empty()
        self._store(*self._form.chunk(*data), track_table(counts), names if names is not None else own)
        return self

    def compress(self, nlist=64, pq_m=64, nprobe=20, train_rows=65536, seed=1234, chunk=1 << 16):
        """A new compact library with this flat library's tracks: an IVF-PQ quantiser trained on a seeded sample of
        train_rows of its own rows (all if there are fewer), every row encoded with it.  This library is left as it is."""
        self._need_flat("compress()")
        self._need_dense("compress()")
        if self.n_rows == 0:
            raise ValueError("compress: the library has no rows to train a quantiser on")
        out = FingerprintLibrary(self.model, self.settings, None, None, precision=self.precision, device=self.device)
        rows = self.rows()
        out._train_quantiser(rows, nlist, pq_m, nprobe, train_rows, seed)
        parts = [out._form.encode(rows[lo:lo + chunk]) for lo in range(0, rows.shape[0], chunk)]
        out._append_codes(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), self.first, self.names)
        return out

    def halve(self, chunk=1 << 18):
        """A new half library with this flat library's tracks: every row rounded to bf16 (round to nearest even,
        ops.rows_to_bf16, `chunk` rows at a time).  From a flat library that keeps every row; this library is left as it
        is.  Against this library a score moves by at most HALF_SCORE_BOUND * max||q|| * max||x||."""
        self._need_flat("halve()", "it is half already")
        self._need_dense("halve()")
        rows = self.rows()
        parts = [ops.rows_to_bf16(rows[lo:lo + chunk]) for lo in range(0, rows.shape[0], chunk)]
        return FingerprintLibrary.from_half(self.model, self.settings,
                                            torch.cat(parts) if parts else rows.to(torch.bfloat16), self.first,
                                            list(self.names), precision=self.precision, device=self.device)

    def thin(self, row_stride):
        """A new flat library that keeps rows first[t] + 0, D, 2D, ... of every track of this dense one (D =
        row_stride): what build(row_stride=D) fingerprints.  This library is left as it is."""
        self._need_flat("thin()")
        self._need_dense("thin()")
        D = int(row_stride)
        if not 1 <= D <= ops.IDENTIFY_MAX_STRIDE:
            raise ValueError(f"row_stride={row_stride} not in [1, {ops.IDENTIFY_MAX_STRIDE}]")
        keep = [np.arange(self.first[t], self.first[t + 1], D) for t in range(self.n_tracks)]
        keep = np.concatenate(keep).astype(np.int64) if keep else np.zeros(0, np.int64)
        rows = self.rows()[torch.from_numpy(keep).to(self.device)]
        return FingerprintLibrary(self.model, self.settings, rows, track_table(-(-np.diff(self.first) // D)),
                                  list(self.names), precision=self.precision, device=self.device, row_stride=D)

    # ---- files -----------------------------------------------------------------------------------------------
    def save(self, out_dir):
        """library.mm + library_shape.npy (the reference's memmap format: eval.load_memmap_data reads them),
        library_tracks.npy (the track table, int64) and library.json (names, settings, precision, model digest).
        A compact library writes library_codes.npy ((n, M) uint8, row order), library_lists.npy ((n) int32),
        library_pq.npz (centroids, codebooks), library_tracks.npy and library.json ("format": 2 and "index": {"type":
        "ivfpq", "nlist", "M", "nprobe"}) -- and no library.mm.  A thinned library writes the flat library's four files
        with "format": 3 and "row_stride": D in library.json.  A half library writes library_half.npy ((n, 128) uint16,
        the bf16 bit patterns), library_tracks.npy and library.json ("format": 5) -- and no library.mm."""
        os.makedirs(out_dir, exist_ok=True)
        meta = {"format": FORMAT, "names": self.names, "settings": self.settings, "precision": self.precision,
                "model_digest": model_digest(self.model), "n_rows": self.n_rows, "n_tracks": self.n_tracks}
        self._form.save(out_dir, self._stored(), meta)
        np.save(os.path.join(out_dir, "library_tracks.npy"), self.first.astype(np.int64))
        with open(os.path.join(out_dir, "library.json"), "w") as f:
            json.dump(meta, f, indent=1)

    @classmethod
    def load(cls, lib_dir, model, device=None, force=False):
        """A library written by save().  Refuses a model whose state_dict digest differs from the one the rows were
        made with, unless force=True."""
        with open(os.path.join(lib_dir, "library.json")) as f:
            meta = json.load(f)
        if meta.get("format") not in (FORMAT, FORMAT_COMPACT, FORMAT_THIN, FORMAT_HALF):
            raise ValueError(f"{lib_dir}: library format {meta.get('format')} is none of {FORMAT}, {FORMAT_COMPACT}, "
                             f"{FORMAT_THIN} and {FORMAT_HALF}")
        stride = meta.get("row_stride", 1 if meta["format"] != FORMAT_THIN else None)
        if meta["format"] == FORMAT_THIN and not (isinstance(stride, int) and 1 <= stride <= ops.IDENTIFY_MAX_STRIDE):
            raise ValueError(f"{lib_dir}: library format {FORMAT_THIN} needs a row_stride in [1, "
                             f"{ops.IDENTIFY_MAX_STRIDE}], not {stride!r}")
        if not force and model_digest(model) != meta["model_digest"]:
            raise ValueError(f"{lib_dir}: the library was fingerprinted with another model (state_dict digest "
                             f"{meta['model_digest'][:12]}...); pass force=True to use it anyway")
        first = np.load(os.path.join(lib_dir, "library_tracks.npy")).astype(np.int64)
        shape, finish = FORMS[meta["format"]].read(lib_dir, meta)
        if shape[0] != int(first[-1]):
            raise ValueError(f"{lib_dir}: {shape[0]} rows but the track table covers {int(first[-1])}")
        if device is not None:
            model = model.to(device)
        lib = cls(model, meta["settings"], None, None, precision=meta["precision"], device=device,
                  row_stride=stride if meta["format"] == FORMAT_THIN else 1)
        lib._form, data = finish(lib.device, lib.row_stride)
        lib._store(*lib._form.chunk(*data), first, meta["names"])
        return lib

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
        return cls(model, cfg, torch.from_numpy(np.ascontiguousarray(rows, np.float32)), track_table(counts), names,
                   precision)

    # ---- the front's hooks -----------------------------------------------------------------------------------
    def _search_rows(self, q, k_probe):
        return self.index.search(q, min(int(k_probe), self.n_rows))[1]

    def _identify_lists(self, q, ids, item_row, item_len, top, min_overlap, max_len, nums=None, q_stride=1,
                        item_ratios=None):
        """One launch of the op of the library's form.  (ShardedFingerprintLibrary runs and merges one per shard.)"""
        dev = self.device
        tail = (torch.from_numpy(self.first).to(dev), q, ids, torch.from_numpy(item_row).to(dev),
                torch.from_numpy(item_len).to(dev))
        kw = dict(top=top, min_overlap=min_overlap, max_len=max_len)
        if q_stride != 1:                                            # (the front refused tempo and the other forms)
            return ops.identify_stride(self.rows(), *tail, q_stride, **kw)
        if nums is not None and item_ratios is not None:
            return ops.identify_tempo_items(self.rows(), *tail, nums, *item_ratios, **kw)
        if nums is not None:
            return ops.identify_tempo(self.rows(), *tail, nums, **kw)
        return self._form.identify(self._stored(), *tail, **kw)

    def _match_lists(self, qb, src, k_probe, nums, kw):
        return self._match_launch(qb, src, self._search_rows(qb, k_probe), nums, kw)

    def _match_launch(self, qb, src, ids, nums, kw):
        """The launch of _match_lists over the hits ids.  (ShardedFingerprintLibrary runs one per shard and merges
        them.)"""
        first_d = torch.from_numpy(self.first).to(self.device)
        if nums is not None:
            return ops.cross_match_tempo(self.rows(), first_d, qb, src, ids, nums, **kw)
        return self._form.cross_match(self._stored(), first_d, qb, src, ids, **kw)

    # ---- the catalog itself ------------------------------------------------------------------------------------
    def self_matches(self, k_probe=32, min_overlap_s=3.0, min_votes=4, min_score=None, top=8, tracks=None,
                     batch_rows=1 << 18, tempo=None, tempo_step=None):
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
        sized workspace (ops.self_match_workspace_bytes: about 124 KB per 303-row source at k_probe = 32, min_votes 4).
        tempo: None, or the speeds to search for tracks that share audio at another speed (a sped-up re-release, a
        varispeed remaster), as match() takes them: a float x for the ratios [1 - x, 1 + x] of track_b rows per track_a
        row, or a pair (lo, hi); tempo_step: the ratio grid's spacing in 1/256, by default 1 for match()'s reason
        (tracks are long: at a coarser grid the nearest ratio drifts off a long span).  The launches then go to
        ops.self_match_tempo (csrc/selfmatch_tempo.hip), R ratios at once, in batches of about batch_rows // R rows (the
        workspace is R times a dense launch's), and row i of track_a sits on row offset + w(i) of track_b, w(i) = (i *
        tempo_num + 128) >> 8.  Each entry then also carries tempo (= tempo_num / 256), tempo_num and b_overlap_s =
        (w(i_hi) - w(i_lo) + 1) segment hops, track_b's side of the span; b_start_s = (offset + w(i_lo)) hops and
        coverage = max(m / rows of a, (w(i_hi) - w(i_lo) + 1) / rows of b), match()'s rule (at 256: m / the shorter
        track, as without tempo).  A copy at ratio rho is reported from both sides, near rho from the original's rows
        and near 1 / rho from the copy's.  Needs a flat library that keeps every row."""
        self._need_tempo_form("self_matches", tempo)
        self._need_flat("self_matches()")
        self._need_dense("self_matches()")
        nums = None if tempo is None else tempo_ratios(tempo, ops.IDENTIFY_TEMPO_DEN, tempo_step)   # step 1 by default
        T, n = self.n_tracks, self.n_rows
        src = list(range(T)) if tracks is None else sorted({int(t) for t in tracks})
        if src and not 0 <= min(src) <= max(src) < T:
            raise ValueError(f"tracks must lie in [0, {T})")
        if n == 0 or T < 2 or not src:
            return []
        min_overlap = max(1, int(math.ceil(float(min_overlap_s) / self.segment_s - 1e-9)))
        k = min(int(k_probe), n)
        rows, dev = self.rows(), self.device
        first_d = torch.from_numpy(self.first).to(dev)
        ids = torch.full((n, k), -1, dtype=torch.int64, device=dev)
        if nums is not None:
            batch_rows = batch_rows // len(nums)                     # the workspace is R times a dense launch's
        out = []
        for i0, i1 in batch_ranges(np.diff(self.first)[src], batch_rows):
            batch = src[i0:i1]
            g = np.concatenate([np.arange(self.first[t], self.first[t + 1]) for t in batch]).astype(np.int64)
            if g.size:
                g_d = torch.from_numpy(g).to(dev)
                _, hit = self.index.search(rows[g_d], k)
                ids[g_d] = hit
            kw = dict(tracks=torch.tensor(batch, dtype=torch.int64), top=int(top), min_votes=int(min_votes),
                      min_overlap=min_overlap)
            res = ops.self_match(rows, first_d, ids, **kw) if nums is None else \
                ops.self_match_tempo(rows, first_d, ids, nums, **kw)
            out += [self._self_match_entry(*slot)
                    for slot in span_slots(res, batch, nums is not None, min_score, "self_match: track")]
        return out

    def _self_match_entry(self, a, b, d, lo, m, sc, v, num=None):
        """One entry of self_matches() from one slot of the kernel's outputs, as _match_entry makes match()'s, for the
        source track a; num: the winning ratio of ops.self_match_tempo (None: dense)."""
        seg_s = self.segment_s
        la, lb = (max(1, int(self.first[t + 1] - self.first[t])) for t in (a, b))
        w_lo, mb = (lo, m) if num is None else tempo_span(lo, m, num)     # track_b's side of the span, in rows
        entry = {"track_a": a, "name_a": self.names[a], "track_b": b, "name_b": self.names[b],
                 "offset": d, "a_start_s": lo * seg_s, "b_start_s": (d + w_lo) * seg_s,
                 "overlap_s": m * seg_s, "coverage": max(m / la, mb / lb), "score": sc, "votes": v}
        if num is not None:
            entry.update({"tempo": num / ops.IDENTIFY_TEMPO_DEN, "tempo_num": num, "b_overlap_s": mb * seg_s})
        return entry

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
