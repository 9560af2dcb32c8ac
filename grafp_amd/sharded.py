"""A fingerprint library sharded over devices (grafp_amd/library.py's FingerprintLibrary, S of them).

A flat library costs 772 bytes per row, so one device holds so many tracks and no more.  A ShardedFingerprintLibrary
holds S ordinary flat FingerprintLibrary shards: shard s owns the contiguous global tracks [tb[s], tb[s+1]) and with
them the global rows [rb[s], rb[s+1]), resident on devices[s].  The model, the segmentation and the embed live on the
primary device, devices[0].

One query call: the segments are embedded once on the primary device; q goes to every shard's device and each shard
searches its own index (min(k_probe, its rows) hits); the distances and ids + rb[s], padded to k = min(k_probe, n_rows)
with inf / -1, come back to the primary device and ops.merge_topk makes the global hit list; every shard then gets that
list minus rb[s] -- hits outside its rows are now outside [0, n) and the kernels ignore them -- and runs its own,
UNCHANGED identify or cross-match op (dense, thinned or tempo, chosen as FingerprintLibrary chooses); its device lists go
to the primary device, one ops.merge_track_lists launch (csrc/merge_lists.hip) merges them, and the result is read back
once.  A shard's list is the one-card list restricted to the shard's tracks and the shards' tracks are disjoint, so the
merged list is, bit for bit and key for key, what the one-card library over the same tracks returns
(tests/test_gpu_sharded.py).  Every device works on its current stream; there are no side streams.  A shard without
rows launches nothing.

identify, identify_windows, timeline, match, their tempo= forms and StreamMonitor(sharded, channels) work as on the
one-card library: both classes derive from library.LibraryFront, which holds the front of each call, and this one
implements its three hooks -- _search_rows, _identify_lists, _match_lists -- over the shards.  Not built: self_matches
across shards, compact (IVF-PQ) shards, shards in several processes, concurrent shards on one device."""
import json
import os

import numpy as np
import torch

from . import ops
from .library import FingerprintLibrary, LibraryFront, _as_waveforms, model_digest, track_names, track_table

FORMAT_SHARDED = 1           # shards.json
INT_MIN = -2 ** 31
# the ops' outputs as merge_track_lists takes them: which are track and score, which travel as payload, and their padding
_IDENTIFY_FORM = dict(track=0, score=2, payload=(1, 3, 4), pad=(INT_MIN, 0, 0))               # offset, votes, ratio
_MATCH_FORM = dict(track=0, score=4, payload=(1, 2, 3, 5, 6), pad=(INT_MIN, -1, 0, 0, 0))    # delta, start, len, votes, ratio


def split_tracks(first, n_shards):
    """The split rule: tb (n_shards + 1 track numbers) with tb[0] = 0, tb[S] = T and otherwise tb[s] the first track
    that starts at or after row s * n_rows / S -- balanced by rows, cut only at track boundaries, shards may be empty."""
    first = np.asarray(first, np.int64).reshape(-1)
    S, T, n = int(n_shards), len(first) - 1, int(first[-1])
    if S < 1:
        raise ValueError(f"n_shards={n_shards} must be at least 1")
    inner = [int(np.searchsorted(first[:T], s * n / S, side="left")) for s in range(1, S)]
    return np.array([0] + inner + [T], np.int64)


def _shard(model, settings, rows, first, names, precision, device, row_stride):
    """One shard.  A shard without tracks has no table to append (FingerprintLibrary refuses a table of one entry)."""
    if len(first) < 2:
        rows = first = names = None
    return FingerprintLibrary(model, settings, rows, first, names, precision=precision, device=device,
                              row_stride=row_stride)


def _cut(lib, t0, t1, device):
    """The tracks [t0, t1) of a flat library as a library of their own on `device`, with its own copy of the rows."""
    r0, r1 = int(lib.first[t0]), int(lib.first[t1])
    rows = lib.rows()[r0:r1]
    rows = rows.clone() if rows.device == torch.device(device) else rows.to(device)
    return _shard(lib.model, lib.settings, rows, lib.first[t0:t1 + 1] - r0, lib.names[t0:t1], lib.precision, device,
                  lib.row_stride)


class ShardedFingerprintLibrary(LibraryFront):
    """S flat FingerprintLibrary shards over contiguous track ranges, queried as one library."""
    is_compact = False

    def __init__(self, shards):
        shards = list(shards)
        if not 1 <= len(shards) <= ops.MERGE_LISTS_MAX:
            raise ValueError(f"{len(shards)} shards, not 1 to {ops.MERGE_LISTS_MAX}")
        head = shards[0]
        for sh in shards:
            if sh.is_half:
                raise NotImplementedError("a sharded library needs flat shards (f32 rows): shards of the half form "
                                          "(bf16 rows) are not built; build the shards with index='flat'")
            if sh.is_compact:
                raise NotImplementedError("a sharded library needs flat shards (f32 rows): compact shards under one "
                                          "shared quantiser are not built")
            if sh.settings != head.settings or sh.precision != head.precision or sh.row_stride != head.row_stride or \
                    sh.model is not head.model:
                raise ValueError("the shards of a library share one model, its settings, precision and row_stride")
        super().__init__(head.model, head.settings, head.precision, head.device, head.row_stride)
        self.shards = shards
        self._refresh()

    def _refresh(self):
        """The global tables from the shards': tb, rb, first and names."""
        self.tb = track_table([sh.n_tracks for sh in self.shards])
        self.rb = track_table([sh.n_rows for sh in self.shards])
        self.first = np.concatenate([sh.first[:-1] + self.rb[s] for s, sh in enumerate(self.shards)] +
                                    [self.rb[-1:]]).astype(np.int64)
        self.names = [name for sh in self.shards for name in sh.names]

    # ---- making one --------------------------------------------------------------------------------------------
    @classmethod
    def split(cls, lib, n_shards, devices=None):
        """The tracks of a flat library (dense or thinned) cut into n_shards shards by split_tracks' rule; shard s on
        devices[s] (default: all on the library's device); every shard gets its own copy of its rows and `lib` is left as
        it is."""
        if lib.is_half:
            raise NotImplementedError("ShardedFingerprintLibrary.split needs the flat form of a library: this one is of "
                                      "the half form (bf16 rows), which is not sharded yet; split the flat library")
        if lib.is_compact:
            raise NotImplementedError("ShardedFingerprintLibrary.split needs the flat form of a library: this one is "
                                      "compact, and IVF-PQ codes under one shared quantiser are not sharded yet")
        devices = cls._devices(devices, n_shards, lib.device)
        tb = split_tracks(lib.first, len(devices))
        return cls(_cut(lib, int(tb[s]), int(tb[s + 1]), dev) for s, dev in enumerate(devices))

    @staticmethod
    def _devices(devices, n_shards, default):
        if devices is None:
            if n_shards is None:
                raise ValueError("give n_shards or devices")
            devices = [default] * int(n_shards)
        devices = [torch.device(d) for d in devices]
        if n_shards is not None and len(devices) != int(n_shards):
            raise ValueError(f"{len(devices)} devices for n_shards={n_shards}")
        if not 1 <= len(devices) <= ops.MERGE_LISTS_MAX:
            raise ValueError(f"{len(devices)} shards, not 1 to {ops.MERGE_LISTS_MAX}")
        return devices

    @classmethod
    def build(cls, model, tracks, cfg, n_shards=None, devices=None, rows_per_shard=None, **kw):
        """Fingerprint whole tracks (as FingerprintLibrary.build takes them, with its keywords: names, precision,
        max_segments, row_stride) on the primary device into shards.  Without rows_per_shard: one
        FingerprintLibrary.build, then split() -- the same rule, stated once.  With it: the model calls are packed as
        FingerprintLibrary.build packs them and a shard is closed, and moved to its device, once it holds at least
        rows_per_shard rows; the last shard takes what is left, so the rows never exist on one device at once."""
        if kw.get("index", "flat") != "flat":
            raise NotImplementedError("ShardedFingerprintLibrary.build: compact shards are not built (index='flat' only)")
        kw.pop("index", None)
        if rows_per_shard is None:
            return cls.split(FingerprintLibrary.build(model, tracks, cfg, **kw), n_shards, devices)
        if int(rows_per_shard) < 1:
            raise ValueError(f"rows_per_shard={rows_per_shard} must be at least 1")
        front = FingerprintLibrary(model, cfg, None, None, precision=kw.get("precision", "bf16"),
                                   row_stride=kw.get("row_stride", 1))
        devices = cls._devices(devices, n_shards, front.device)
        waves, own = _as_waveforms(tracks)
        names = track_names(kw.get("names") if kw.get("names") is not None else own, len(waves))
        shards, parts, held, t0, counts = [], [], [], 0, []

        def close(t1):
            rows = torch.cat(parts) if parts else torch.zeros((0, 128), device=front.device)
            shards.append(_shard(model, cfg, rows, track_table(held), names[t0:t1], front.precision,
                                 devices[len(shards)], front.row_stride))
            parts.clear()
            held.clear()

        done = 0                                                     # tracks whose rows have been handed to a shard
        for rows in front._fingerprint_batches(waves, int(kw.get("max_segments", 4096)), counts):
            r0 = 0
            for t in range(done, len(counts)):                       # (a model call holds whole tracks)
                parts.append(rows[r0:r0 + counts[t]])
                held.append(counts[t])
                r0 += counts[t]
                if sum(held) >= int(rows_per_shard) and len(shards) < len(devices) - 1:
                    close(t + 1)
                    t0 = t + 1
            done = len(counts)
        held += counts[done:]                                        # (trailing tracks without rows)
        close(len(waves))
        while len(shards) < len(devices):
            t0 = len(waves)
            close(len(waves))
        return cls(shards)

    def add(self, tracks, names=None, max_segments=4096):
        """Append tracks (as for build) to the last shard: fingerprinted on the primary device, the global order stays
        contiguous.  rebalance() evens the shards out again."""
        waves, own = _as_waveforms(tracks)
        names = track_names(names if names is not None else own, len(waves), self.n_tracks)
        rows, counts = self._fingerprint_tracks(waves, int(max_segments))
        self.shards[-1]._append(rows, track_table(counts), names)
        self._refresh()
        return self

    def _whole(self):
        """All shards' tracks as one library on the primary device."""
        rows = torch.cat([sh.rows().to(self.device) for sh in self.shards])
        return FingerprintLibrary(self.model, self.settings, rows, self.first, self.names, precision=self.precision,
                                  device=self.device, row_stride=self._row_stride)

    def rebalance(self):
        """split() of the concatenation, onto the same devices (the rows pass through the primary device)."""
        self.shards = type(self).split(self._whole(), None, [sh.device for sh in self.shards]).shards
        self._refresh()
        return self

    # ---- files -------------------------------------------------------------------------------------------------
    def save(self, out_dir):
        """shards.json ({"format", "n_shards", "tb", "shards": directory names, "model_digest"}) and one ordinary
        FingerprintLibrary.save directory per shard."""
        os.makedirs(out_dir, exist_ok=True)
        dirs = [f"shard{s:03d}" for s in range(len(self.shards))]
        for sh, d in zip(self.shards, dirs):
            sh.save(os.path.join(out_dir, d))
        with open(os.path.join(out_dir, "shards.json"), "w") as f:
            json.dump({"format": FORMAT_SHARDED, "n_shards": len(dirs), "tb": [int(v) for v in self.tb], "shards": dirs,
                       "model_digest": model_digest(self.model)}, f, indent=1)

    @staticmethod
    def is_sharded_dir(lib_dir):
        return os.path.exists(os.path.join(lib_dir, "shards.json"))

    @classmethod
    def load(cls, lib_dir, model, devices=None, force=False):
        """A library written by save(); shard s on devices[s] (default: all on the model's device).  Refuses a model
        whose state_dict digest differs from the one the rows were made with, unless force=True."""
        with open(os.path.join(lib_dir, "shards.json")) as f:
            meta = json.load(f)
        dirs, tb = meta.get("shards"), meta.get("tb")
        if meta.get("format") != FORMAT_SHARDED or not isinstance(dirs, list) or not isinstance(tb, list) or \
                meta.get("n_shards") != len(dirs) or len(tb) != len(dirs) + 1 or not dirs or \
                not all(isinstance(d, str) and d and os.path.basename(d) == d for d in dirs) or \
                not all(isinstance(v, int) for v in tb) or tb[0] != 0 or any(b < a for a, b in zip(tb, tb[1:])):
            raise ValueError(f"{lib_dir}: shards.json is no format {FORMAT_SHARDED} table of shard directories and "
                             "ascending track bases")
        if not force and model_digest(model) != meta.get("model_digest"):
            raise ValueError(f"{lib_dir}: the library was fingerprinted with another model (state_dict digest "
                             f"{str(meta.get('model_digest'))[:12]}...); pass force=True to use it anyway")
        if devices is not None:
            model = model.to(torch.device(devices[0]))
        devices = cls._devices(devices, len(dirs), next(model.parameters()).device)
        shards = []
        for s, (d, dev) in enumerate(zip(dirs, devices)):
            if tb[s + 1] == tb[s]:                                   # no tracks: its library.json says all there is
                with open(os.path.join(lib_dir, d, "library.json")) as f:
                    sub = json.load(f)
                n_tracks = sub.get("n_tracks")
                sh = _shard(model, sub["settings"], None, [0], None, sub["precision"], dev, sub.get("row_stride", 1))
            else:
                sh = FingerprintLibrary.load(os.path.join(lib_dir, d), model, None, force=force)  # on the model's device
                n_tracks = sh.n_tracks
            if n_tracks != tb[s + 1] - tb[s]:
                raise ValueError(f"{lib_dir}: shard {d} holds {n_tracks} tracks, shards.json says "
                                 f"{tb[s + 1] - tb[s]}")
            shards.append(sh if sh.device == dev else _cut(sh, 0, sh.n_tracks, dev))
        return cls(shards)

    @property
    def nbytes(self):
        """Device bytes over all shards (FingerprintLibrary.nbytes of each)."""
        return int(sum(sh.nbytes for sh in self.shards))

    # ---- queries: LibraryFront's calls (the one-card library's signatures, defaults, result dicts and refusals) ------
    def self_matches(self, *args, **kw):
        raise NotImplementedError("ShardedFingerprintLibrary.self_matches is not built: it needs the S^2 shard pairs "
                                  "through _match_rows")

    def _live(self):
        """(s, shard) of the shards that hold rows: the others launch nothing."""
        return [(s, sh) for s, sh in enumerate(self.shards) if sh.n_rows]

    def _search_rows(self, q, k_probe):
        """The global hits of the rows q: every shard's own search, merged on the primary device by (distance, id)."""
        k = min(int(k_probe), self.n_rows)
        dist, ids = [], []
        for s, sh in self._live():
            with torch.cuda.device(sh.device):
                d, i = sh.index.search(q.to(sh.device), min(k, sh.n_rows))
                i = torch.where(i >= 0, i + int(self.rb[s]), i)
                fill = k - d.shape[1]
                if fill:
                    d = torch.nn.functional.pad(d, (0, fill), value=float("inf"))
                    i = torch.nn.functional.pad(i, (0, fill), value=-1)
            dist.append(d.to(self.device))
            ids.append(i.to(self.device))
        with torch.cuda.device(self.device):
            return ops.merge_topk(torch.stack(dist), torch.stack(ids))[1]

    def _merge(self, outs, live, form):
        """The shards' op outputs (tuples of device tensors, in the op's own order) -> one tuple in that order on the
        primary device: one ops.merge_track_lists launch."""
        n_out = len(outs[0])
        payload = [j for j in form["payload"] if j < n_out]
        gather = lambda j: torch.stack([o[j].to(self.device) for o in outs])
        with torch.cuda.device(self.device):
            tr, sc, pl = ops.merge_track_lists(gather(form["track"]), gather(form["score"]),
                                               torch.stack([gather(j) for j in payload]),
                                               [int(self.tb[s]) for s, _ in live], form["pad"][:len(payload)])
        merged = {form["track"]: tr, form["score"]: sc, **{j: pl[p] for p, j in enumerate(payload)}}
        return tuple(merged[j] for j in range(n_out))

    def _on_shards(self, q, ids, launch, form):
        """launch(shard, q, ids) on every shard that holds rows, on its device, with the rows q and the global hits ids
        minus the shard's row base moved there; the shards' lists merged."""
        live, outs = self._live(), []
        for s, sh in live:
            with torch.cuda.device(sh.device):
                outs.append(launch(sh, q.to(sh.device), (ids - int(self.rb[s])).to(sh.device)))
        return self._merge(outs, live, form)

    def _identify_lists(self, q, ids, item_row, item_len, top, min_overlap, max_len, nums=None, q_stride=1,
                        item_ratios=None):
        """FingerprintLibrary._identify_lists on every shard that holds rows."""
        kw = {} if item_ratios is None else {"item_ratios": item_ratios}
        return self._on_shards(q, ids, lambda sh, q_s, ids_s: sh._identify_lists(
            q_s, ids_s, item_row, item_len, top, min_overlap, max_len, nums, q_stride, **kw), _IDENTIFY_FORM)

    def _match_lists(self, qb, src, k_probe, nums, kw):
        """One merged search, then FingerprintLibrary._match_launch on every shard over the same batch of recordings."""
        return self._on_shards(qb, self._search_rows(qb, k_probe), lambda sh, q_s, ids_s: sh._match_launch(
            q_s, src, ids_s, nums, kw), _MATCH_FORM)
