"""Device-resident training corpus: the real-audio replacement of the reference's NeuralfpDataset (modules/data.py).

The reference decodes, resamples and quantile-normalises every track on DataLoader workers, per item and on the CPU
(modules/data.py:45-89).  DeviceAudioCorpus does that work once: the host decodes every track (PCM WAV at any rate and
channel count, or .npy), the tracks are uploaded in bounded chunks and resampled to cfg['fs'] on the device
(ops.resample, csrc/corpus.hip), and they stay in HBM as one ragged bank (flat f32 buffer + per-track start and
length, the layout of the augmentation banks).  Each training step then draws a whole batch of (x_i, x_j) crops in one
launch (ops.draw_pairs), following NeuralfpDataset.__getitem__ for training; evaluation reads whole resampled tracks
(tracks()), which fpdb.create_fp_db / create_dummy_db take in place of DataLoader(NeuralfpDataset(train=False)).

Differences from the reference, on purpose:
  * a track shorter than offset_mod + 1 samples (offset_mod = int(fs*offset + clip); with speed or time-stretch
    augmentation on, int(fs*offset) + draw_len: the views are drawn with the context those need) is excluded from
    training draws and counted (stats['excluded']).  The reference skips tracks up to one clip long (:61-62) and raises in
    np.random.randint for those up to offset_mod (:74); here neither happens.
  * a silent draw moves on to the next track of the corpus (order of the index), as `self[idx + 1]` does, but at most
    `attempts` times; if all are silent the last draw is used and counted (silent_rows()).
  * mp3 is not decoded (no decoder on this image): an mp3 entry uses a .wav or .npy with the same stem if one exists,
    otherwise it is reported and refused, or skipped with skip_undecodable=True.
"""
import collections
import glob
import json
import math
import os
import struct
import time

import numpy as np
import torch

from . import ops

_DECODABLE = (".wav", ".npy")


# ---------------------------------------------------------------------------------------------------------------------
# host decoding
# ---------------------------------------------------------------------------------------------------------------------
def _wav_header(path):
    """(format tag, channels, rate, bits per sample, data offset, data bytes) of a RIFF/WAVE file."""
    with open(path, "rb") as f:
        riff = f.read(12)
        if len(riff) < 12 or riff[:4] != b"RIFF" or riff[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        fmt = None
        while True:
            hdr = f.read(8)
            if len(hdr) < 8:
                raise ValueError(f"{path}: no data chunk")
            cid, size = hdr[:4], struct.unpack("<I", hdr[4:])[0]
            if cid == b"fmt ":
                body = f.read(size + (size & 1))
                tag, ch, rate, _, _, bits = struct.unpack("<HHIIHH", body[:16])
                if tag == 0xFFFE and size >= 26:              # WAVE_FORMAT_EXTENSIBLE: the sub-format's first word
                    tag = struct.unpack("<H", body[24:26])[0]
                fmt = (tag, ch, rate, bits)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: data chunk before fmt chunk")
                return fmt + (f.tell(), size)
            else:
                f.seek(size + (size & 1), 1)


def wav_info(path):
    """(sample rate, frames) from the header alone."""
    tag, ch, rate, bits, _, size = _wav_header(path)
    return rate, size // (ch * (bits // 8))


def read_wav(path):
    """A PCM (8, 16, 24, 32-bit integer) or IEEE-float (32-bit) WAV file -> ((channels, frames) float32, rate), scaled as
    torchaudio.load does: unsigned 8-bit (x - 128) / 128, signed n-bit x / 2^(n-1)."""
    tag, ch, rate, bits, off, size = _wav_header(path)
    width = bits // 8
    n = size // (ch * width)
    with open(path, "rb") as f:
        f.seek(off)
        raw = f.read(n * ch * width)
    if tag == 3 and bits == 32:
        a = np.frombuffer(raw, dtype="<f4").astype(np.float32)
    elif tag != 1:
        raise ValueError(f"{path}: unsupported WAV format tag {tag}")
    elif bits == 8:
        a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif bits == 16:
        a = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif bits == 24:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        a = v.astype(np.float32) / 8388608.0
    elif bits == 32:
        a = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    else:
        raise ValueError(f"{path}: unsupported PCM sample width {bits} bits")
    return a.reshape(n, ch).T, rate


def _mono(a):
    """audio.mean(dim=0) of a (channels, frames) array, as the reference downmixes (float32, torch's reduction)."""
    a = np.asarray(a, dtype=np.float32)
    if a.ndim == 1:
        return a
    if a.shape[0] == 1:
        return a[0].copy()
    return torch.from_numpy(np.ascontiguousarray(a)).mean(dim=0).numpy()


def read_audio(path, npy_fs):
    """One mono float32 recording and its rate from a .wav or .npy file (.npy: (frames,) or (channels, frames) at
    npy_fs)."""
    if path.lower().endswith(".npy"):
        return _mono(np.load(path)), int(npy_fs)
    a, rate = read_wav(path)
    return _mono(a), rate


def _probe(path, npy_fs):
    """(rate, frames) of a decodable file without decoding it."""
    if path.lower().endswith(".npy"):
        a = np.load(path, mmap_mode="r")
        return int(npy_fs), int(a.shape[-1])
    return wav_info(path)


def resolve_files(paths, skip_undecodable=False):
    """Entries that cannot be decoded here (mp3 and any other extension) -> the .wav or .npy with the same stem if one
    exists.  -> (files, report) with report = {'substituted': n, 'skipped': [paths]}.  Refuses (ValueError, with the
    counts) when something is left undecodable and skip_undecodable is False."""
    files, substituted, left = [], 0, []
    for p in paths:
        if p.lower().endswith(_DECODABLE):
            files.append(p)
            continue
        stem = os.path.splitext(p)[0]
        alt = next((stem + e for e in _DECODABLE if os.path.exists(stem + e)), None)
        if alt is None:
            left.append(p)
        else:
            files.append(alt)
            substituted += 1
    if left and not skip_undecodable:
        exts = collections.Counter(os.path.splitext(p)[1].lower() or "(none)" for p in left)
        raise ValueError(f"{len(left)} of {len(paths)} tracks cannot be decoded here ({dict(exts)}; only PCM .wav and "
                         f".npy are; {substituted} were replaced by a .wav/.npy of the same stem), e.g. {left[0]}. "
                         "Convert them, or pass skip_undecodable=True to leave them out.")
    return files, {"substituted": substituted, "skipped": left}


def list_source(source):
    """File list of a source: a directory (recursive .wav / .npy, sorted), the reference's JSON index
    ({"0": path, ...}, in index order, as util.load_index + NeuralfpDataset read it), one file, or a list of files."""
    if isinstance(source, str):
        if os.path.isdir(source):
            return sorted(glob.glob(os.path.join(source, "**", "*.wav"), recursive=True) +
                          glob.glob(os.path.join(source, "**", "*.npy"), recursive=True))
        if source.endswith(".json"):
            with open(source) as fp:
                index = json.load(fp)
            keys = list(index)
            if all(str(k).isdigit() for k in keys):
                keys = sorted(keys, key=int)
            return [index[k] for k in keys]
        return [source]
    return [str(p) for p in source]


# ---------------------------------------------------------------------------------------------------------------------
# epoch plan
# ---------------------------------------------------------------------------------------------------------------------
def epoch_plan(n, batch, generator=None, rank=0, world=1):
    """Rows of rank `rank` for one epoch over n tracks: a permutation shared by all ranks (same generator seed ->
    same permutation), cut into steps of world * batch; rank r takes slice r of every step; the last partial step is
    dropped (DataLoader(shuffle=True, drop_last=True)).  -> list of (batch,) int64 CPU tensors."""
    if batch <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError("epoch_plan: bad batch / rank / world")
    dev = generator.device if generator is not None else "cpu"
    perm = torch.randperm(n, generator=generator, device=dev).cpu()
    steps = n // (batch * world)
    return [perm[(s * world + rank) * batch:(s * world + rank + 1) * batch] for s in range(steps)]


# ---------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------
def _quantile(v, q):
    """torch.quantile(v, q) (linear interpolation, float32) also past the size limit of torch.quantile (2^24)."""
    if v.numel() <= (1 << 24):
        return torch.quantile(v, q)
    s = torch.sort(v).values
    rank = torch.tensor(q, dtype=v.dtype, device=v.device) * (v.numel() - 1)
    lo = rank.long()
    hi = rank.ceil().long()
    return torch.lerp(s[lo], s[hi], rank - lo)


class _Tracks:
    """Indexable sequence of (1, T) device views of resampled tracks (what DataLoader(NeuralfpDataset(train=False),
    batch_size=1) yields), for fpdb.create_fp_db / create_dummy_db, including their world > 1 indexing."""

    def __init__(self, corpus, indices):
        self._c, self._idx = corpus, [int(i) for i in indices]

    def __len__(self):
        return len(self._idx)

    def __getitem__(self, i):
        return self._c.track(self._idx[i]).view(1, -1)

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class DeviceAudioCorpus:
    """Tracks decoded once, resampled to cfg['fs'] on the device and resident in HBM as a ragged bank.

    source: a directory (recursive .wav / .npy), a list of files, the reference's JSON index, or arrays: a 2-D array /
      tensor (rows = tracks) or a list of 1-D ones, at rate `fs` (default cfg['fs']); a list of (array, rate) pairs.
    npy_fs: rate of .npy files (default cfg['fs']).  chunk_bytes: source audio uploaded per resample launch.
    skip_undecodable: leave out (and count) tracks that cannot be decoded instead of refusing the source."""

    def __init__(self, cfg, source, device, fs=None, npy_fs=None, skip_undecodable=False, chunk_bytes=1 << 30,
                 verbose=False):
        self.cfg, self.device = cfg, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceAudioCorpus lives on a HIP device: no CPU corpus (the reference's CPU path is "
                               "modules/data.py)")
        self.fs = int(cfg["fs"])
        self.clip = int(self.fs * cfg["dur"])
        self.offset_mod = int(self.fs * cfg["offset"] + self.clip)
        # speed augmentation on (cfg['speed_prob'] > 0): both views are drawn at draw_len samples, the clip plus the context
        # ops.speed_change needs at the largest ratio; the jitter between the views stays int(fs * offset)
        # time-stretch augmentation on (cfg['stretch_prob'] > 0): draw_len also holds what ops.time_stretch needs to
        # produce the speed change's input (or the clip): ops.view_plan, which GPUTransformNeuralfp.draw_len comes from too
        plan = ops.view_plan(cfg)
        self.draw_len = plan.draw_len
        if plan.on:
            self.offset_mod = int(self.fs * cfg["offset"]) + self.draw_len
            if self.offset_mod > ops.DRAW_PAIRS_MAX_WINDOW:
                keys = " and ".join(f"{k} = {list(cfg[k])}" for k, on in (("stretch_range", plan.stretch),
                                                                         ("speed_range", plan.speed)) if on is not None)
                raise ValueError(f"{keys}: the training draw needs a window of "
                                 f"{self.offset_mod} samples (draw_len = {self.draw_len} plus the offset jitter), more than "
                                 f"the {ops.DRAW_PAIRS_MAX_WINDOW} draw_pairs holds on chip; lower the upper ratio, dur or offset")
        self.silence = float(cfg["silence"])
        self.norm_q = cfg.get("norm")
        npy_fs = self.fs if npy_fs is None else int(npy_fs)
        t0 = time.perf_counter()
        timing = collections.Counter()

        # (rate, frames, loader) per track, in source order
        entries, report = [], {"substituted": 0, "skipped": []}
        if isinstance(source, (np.ndarray, torch.Tensor)) or (
                isinstance(source, (list, tuple)) and source and not isinstance(source[0], str)):
            rate = self.fs if fs is None else int(fs)
            rows = source if not (isinstance(source, (np.ndarray, torch.Tensor)) and source.ndim == 1) else [source]
            for r in rows:
                if isinstance(r, tuple):
                    r, r_fs = r
                else:
                    r_fs = rate
                a = (r.detach().cpu().numpy() if isinstance(r, torch.Tensor) else np.asarray(r)).astype(np.float32).reshape(-1)
                entries.append((int(r_fs), a.size, (lambda a=a: a)))
            self.files = None
        else:
            files, report = resolve_files(list_source(source), skip_undecodable)
            for p in files:
                rate, frames = _probe(p, npy_fs)
                entries.append((rate, frames, (lambda p=p: read_audio(p, npy_fs)[0])))
            self.files = files
        if not entries:
            raise ValueError("DeviceAudioCorpus: no tracks in the source")
        timing["probe"] += time.perf_counter() - t0

        n = len(entries)
        out_len = [ops.resampled_length(fr, r, self.fs) for r, fr, _ in entries]
        starts = np.concatenate([[0], np.cumsum(out_len[:-1], dtype=np.int64)]).astype(np.int64)
        self.bank = torch.empty(max(int(sum(out_len)), 1), dtype=torch.float32, device=self.device)
        # per source rate, chunks of about chunk_bytes of source audio: decode, upload, one resample launch, free
        by_rate = collections.defaultdict(list)
        for i, (r, _, _) in enumerate(entries):
            by_rate[r].append(i)
        for rate, ids in by_rate.items():
            lo = 0
            while lo < len(ids):
                hi, size = lo, 0
                while hi < len(ids) and (hi == lo or size + 4 * entries[ids[hi]][1] <= chunk_bytes) and hi - lo < 65535:
                    size += 4 * entries[ids[hi]][1]
                    hi += 1
                chunk = ids[lo:hi]
                t = time.perf_counter()
                arrays = [entries[i][2]() for i in chunk]
                for i, a in zip(chunk, arrays):
                    if a.size != entries[i][1]:
                        raise ValueError(f"track {i}: header says {entries[i][1]} frames, decoded {a.size}")
                flat = np.concatenate(arrays) if arrays else np.zeros(0, np.float32)
                lens = np.array([a.size for a in arrays], dtype=np.int64)
                del arrays
                timing["decode"] += time.perf_counter() - t
                t = time.perf_counter()
                src = torch.from_numpy(flat).to(self.device)
                del flat
                torch.cuda.synchronize(self.device)
                timing["upload"] += time.perf_counter() - t
                t = time.perf_counter()
                in_starts = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
                if src.numel() > 0:
                    ops.resample(src, torch.from_numpy(in_starts), torch.from_numpy(lens), rate, self.fs, out=self.bank,
                                 out_starts=torch.from_numpy(starts[chunk]))
                torch.cuda.synchronize(self.device)
                del src                                   # the source-rate copy of this chunk
                timing["resample"] += time.perf_counter() - t
                lo = hi

        self.track_start = torch.from_numpy(starts).to(self.device)
        self.track_len = torch.tensor(out_len, dtype=torch.int64, device=self.device)
        self._len_h = list(out_len)
        self._start_h = starts.tolist()
        t = time.perf_counter()
        if self.norm_q is None:
            self.norms = torch.ones(n, dtype=torch.float32, device=self.device)
        else:
            self.norms = torch.stack([1e-8 + _quantile(self.track(i).abs(), float(self.norm_q)) if out_len[i] > 0 else
                                      torch.ones((), dtype=torch.float32, device=self.device) for i in range(n)])
        torch.cuda.synchronize(self.device)
        timing["quantile"] += time.perf_counter() - t

        self.eligible = [i for i in range(n) if out_len[i] >= self.offset_mod + 1]
        self._pos = {t: k for k, t in enumerate(self.eligible)}
        el = torch.tensor(self.eligible, dtype=torch.int64, device=self.device)
        self._el_start, self._el_len, self._el_norm = self.track_start[el], self.track_len[el], self.norms[el]
        self._silent = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.stats = {
            "tracks": n,
            "seconds": float(sum(out_len)) / self.fs,
            "excluded": n - len(self.eligible),
            "rates": dict(collections.Counter(r for r, _, _ in entries)),
            "substituted": report["substituted"],
            "undecodable": len(report["skipped"]),
            "load_s": dict(timing, total=time.perf_counter() - t0),
        }
        if verbose:
            print(f"DeviceAudioCorpus: {self.stats}")

    # ---- sizes and views ------------------------------------------------------------------------------------
    def __len__(self):
        return len(self._len_h)

    def track(self, i):
        """Resampled track i: a 1-D device view into the bank."""
        s = self._start_h[i]
        return self.bank[s:s + self._len_h[i]]

    def tracks(self, indices=None):
        """(1, T) device tracks for fingerprinting.  indices=None: every track longer than one clip (the reference's
        dataset substitutes the next track for the others, modules/data.py:61-62)."""
        if indices is None:
            indices = [i for i in range(len(self)) if self._len_h[i] > self.clip]
        return _Tracks(self, indices)

    def silent_rows(self):
        """Rows written so far whose every attempt was silent."""
        return int(self._silent.item())

    # ---- training draws -------------------------------------------------------------------------------------
    def draw_pairs(self, track_ids, generator=None, attempts=8):
        """One batch: row b starts at corpus track track_ids[b] (which must be eligible) -> (x_i, x_j), (B, draw_len):
        draw_len is the clip, or with speed or time-stretch augmentation on the clip plus their context (what
        GPUTransformNeuralfp.forward and Trainer.step then take)."""
        try:
            rows = [self._pos[int(t)] for t in torch.as_tensor(track_ids).reshape(-1).tolist()]
        except KeyError as e:
            raise ValueError(f"track {e.args[0]} is shorter than offset_mod + 1 = {self.offset_mod + 1} samples and "
                             "excluded from training draws") from None
        return self._draw(torch.tensor(rows, dtype=torch.int32), generator, attempts)

    def _draw(self, rows, generator, attempts):
        B = rows.numel()
        gdev = generator.device if generator is not None else self.device
        u = torch.rand((B, attempts, 3), generator=generator, device=gdev).to(self.device)
        return ops.draw_pairs(self.bank, self._el_start, self._el_len, self._el_norm, rows.to(self.device), u, self.draw_len,
                              self.offset_mod, self.silence, self._silent)

    def batches(self, batch, generator=None, rank=0, world=1, attempts=8):
        """One epoch of training batches for rank `rank` of `world`: yields (x_i, x_j) per step (see epoch_plan)."""
        if not self.eligible:
            raise ValueError("no track is long enough for a training draw")
        for rows in epoch_plan(len(self.eligible), batch, generator, rank, world):
            yield self._draw(rows.to(torch.int32), generator, attempts)

    def steps_per_epoch(self, batch, world=1):
        return len(self.eligible) // (batch * world)
