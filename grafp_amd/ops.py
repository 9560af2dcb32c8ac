"""Torch-facing wrappers over the C ABI (include/grafp_hip.h).

PyTorch is used here for device memory, the current HIP stream and autograd plumbing only; every
computation below runs in libgrafp_hip.so.  There is no CPU path: tensors that are not on a HIP device
raise immediately.
"""
import collections
import contextlib
import ctypes
import math
import os

import numpy as np
import torch
from torch.amp import custom_bwd, custom_fwd

from ._lib import check, lib

_vp = ctypes.c_void_p


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "grafp_amd ops run only on a HIP device (MI355X): got a CPU tensor and there is no CPU "
                "fallback by design (the CPU restatement lives in oracle/ and is test infrastructure).")


def _p(t):
    return _vp(t.data_ptr()) if t is not None else None


# the raw handle of torch's current stream, straight from the C bindings: torch.cuda.current_stream() builds a Stream
# object and validates the device on every call (~10 us; 160 launches of a 128-pair step made that 1.6 ms of host time
# per pass -- the eager step is host-bound at that size: tools/host_profile.py)
_raw_stream, _cur_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice


def _stream():
    return _vp(_raw_stream(_cur_device()))


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


class _Switches:
    """A/B switches of the host glue for tests and measurement tools (tests/, tools/): plain attributes read at call
    time and set by the test or tool itself.  The product path reads NO environment variable for its behaviour."""
    bn_two_pass = False           # True: the two-kernel BatchNorm (statistics, then apply) instead of the single pass
    grouped_bmm_min = 128         # f32 mode: channels per group from which a grouped conv runs as a batched library GEMM
    wgrad_f32_library = False     # True: f32 weight gradients by the library GEMM instead of the split-bf16 kernel
    fused_conv_bn = True          # False: library GEMM + fused BatchNorm kernel pair instead of conv1x1_gemm (bf16 mode)
    shortcut_fusion = True        # False: autograd's accumulate kernel instead of the [W^T | I] data-gradient product
    bn_spin_limit = -1            # polls of the single-pass BatchNorm rendezvous (-1: the library default; 0: never wait)
    knn_split = True              # False: every k-NN graph by the exact-f32 MFMA kernel (knn_graph.hip) -- same indices
    fused_eval_affine = True      # False: eval-mode conv+BN+act as GEMM + normalise pass (same bits) instead of one kernel
    defer_norm = True             # False: every BatchNorm + activation by its own pass (no normalise-on-load at stages 0-1)
    mrconv_arg = True             # False: max-relative backward recomputes the arg-max from x instead of reading the record
    f32_split_gemm = False        # True: the f32 mode's matrix-bound products (>= 256 operand rows) as split-bf16 MFMAs --
    #                               2^-16 instead of 2^-24 per product: faster, but NOT inside the f32 mode's 1e-4 parity bars


switches = _Switches()


# ------------------------------------------------------------------------------------------------
# Optional per-kernel timing with HIP events on the launch stream (bench.py's roofline block)
# ------------------------------------------------------------------------------------------------
_TIMED = {}     # name -> list of (start_event, end_event, meta)


@contextlib.contextmanager
def time_kernels(*names):
    """Record HIP events around every launch of the named ops inside the block.
    Yields a dict name -> list[(start, end, meta)]; call `elapsed_ms(events)` after a synchronize."""
    for n in names:
        _TIMED[n] = []
    try:
        yield _TIMED
    finally:
        for n in names:
            _TIMED.pop(n, None)


@contextlib.contextmanager
def _timed(name, meta=None):
    rec = _TIMED.get(name)
    if rec is None:
        yield
        return
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    yield
    e.record()
    rec.append((s, e, meta))


def elapsed_ms(events):
    return [s.elapsed_time(e) for s, e, _ in events]


# ------------------------------------------------------------------------------------------------
# K1 / K1b  log-mel
# ------------------------------------------------------------------------------------------------
_MEL_PLANS = {}


def mel_filterbank(n_freqs, n_mels, sample_rate, f_min=0.0, f_max=None):
    """HTK triangular filterbank, norm=None, in f32 exactly as torchaudio==2.3.0 builds it
    (`melscale_fbanks`; the reference gets it through MelSpectrogram, modules/transformations.py:51)."""
    f_max = float(sample_rate // 2) if f_max is None else float(f_max)
    freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    mel_lo = 2595.0 * math.log10(1.0 + f_min / 700.0)
    mel_hi = 2595.0 * math.log10(1.0 + f_max / 700.0)
    pts = 700.0 * (10.0 ** (torch.linspace(mel_lo, mel_hi, n_mels + 2) / 2595.0) - 1.0)
    width = pts[1:] - pts[:-1]
    slope = pts.unsqueeze(0) - freqs.unsqueeze(1)
    rising = slope[:, 2:] / width[1:]
    falling = (-1.0 * slope[:, :-2]) / width[:-1]
    return torch.clamp(torch.minimum(falling, rising), min=0.0)


class _MelPlan:
    def __init__(self, device, fs, n_fft, win_len, n_mels):
        win = torch.hann_window(win_len)                       # periodic, as torch.stft's default use
        if win_len < n_fft:
            left = (n_fft - win_len) // 2
            win = torch.nn.functional.pad(win, (left, n_fft - win_len - left))
        j = torch.arange(n_fft // 2, dtype=torch.float64)
        ang = 2.0 * math.pi * j / n_fft
        tw = torch.stack((torch.cos(ang), -torch.sin(ang)), dim=1).to(torch.float32)
        fb = mel_filterbank(n_fft // 2 + 1, n_mels, fs)
        nz = fb > 0
        any_nz = nz.any(dim=0)
        lo = torch.where(any_nz, nz.to(torch.int32).argmax(dim=0), torch.ones(n_mels, dtype=torch.int64))
        hi = torch.where(any_nz, fb.shape[0] - 1 - nz.flip(0).to(torch.int32).argmax(dim=0),
                         torch.zeros(n_mels, dtype=torch.int64))
        self.window = win.to(device).contiguous()
        self.twiddle = tw.to(device).contiguous()
        self.fb = fb.to(device).contiguous()
        self.band_lo = lo.to(torch.int32).to(device).contiguous()
        self.band_hi = hi.to(torch.int32).to(device).contiguous()


def _mel_plan(device, fs, n_fft, win_len, n_mels):
    key = (str(device), fs, n_fft, win_len, n_mels)
    if key not in _MEL_PLANS:
        _MEL_PLANS[key] = _MelPlan(device, fs, n_fft, win_len, n_mels)
    return _MEL_PLANS[key]


def logmel(wav, fs=16000, n_fft=1024, win_len=1024, hop=512, n_mels=64):
    """(B, T) or (T,) waveform -> (B, n_mels, 1 + T // hop) dB (or (n_mels, frames) for 1-D input)."""
    _require_gpu(wav)
    squeeze = wav.dim() == 1
    x = _f32c(wav.reshape(-1, wav.shape[-1]))
    B, T = x.shape
    plan = _mel_plan(x.device, fs, n_fft, win_len, n_mels)
    out = torch.empty((B, n_mels, 1 + T // hop), dtype=torch.float32, device=x.device)
    with _timed("logmel", (B, T)):
        check(lib.grafp_logmel_f32(_p(x), x.stride(0), B, T, n_fft, hop, n_mels, _p(plan.window), _p(plan.twiddle),
                                   _p(plan.fb), _p(plan.band_lo), _p(plan.band_hi), _p(out), _stream()), "logmel")
    return out[0] if squeeze else out


def unfold_segments(spec, size, step):
    """(n_mels, n_frames) -> contiguous (n_seg, n_mels, size); values of
    `spec.transpose(1,0).unfold(0, size, step)` (modules/transformations.py:89-90)."""
    _require_gpu(spec)
    s = _f32c(spec)
    n_mels, n_frames = s.shape
    if n_frames < size:
        return torch.empty((0, n_mels, size), dtype=torch.float32, device=s.device)
    n_seg = (n_frames - size) // step + 1
    seg = torch.empty((n_seg, n_mels, size), dtype=torch.float32, device=s.device)
    check(lib.grafp_unfold_segments_f32(_p(s), n_mels, n_frames, size, step, _p(seg), _stream()), "unfold_segments")
    return seg


# ------------------------------------------------------------------------------------------------
# K1 for live streams (csrc/stream_frontend.hip; grafp_amd/monitor.py holds the per-channel state)
# ------------------------------------------------------------------------------------------------
STREAM_PAIRS_PER_GROUP = 8          # frame pairs of one channel a workgroup of stream_logmel does (LM1K_PAIRS)


def _host_i64(v, n, what):
    a = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v).astype(np.int64).reshape(-1)
    if a.shape[0] != n:
        raise ValueError(f"{what}: {a.shape[0]} entries for {n} channels")
    return a


def _check_ring(name, ring, n_mels=None):
    if ring.dim() != 3 or ring.dtype != torch.float32 or not ring.is_contiguous():
        raise ValueError(f"{name}: the ring must be a contiguous f32 (channels, n_mels, R) tensor")
    R = int(ring.shape[2])
    if R < 2 or R & (R - 1) or (n_mels is not None and int(ring.shape[1]) != int(n_mels)):
        raise ValueError(f"{name}: a ring of shape {tuple(ring.shape)} needs R a power of two"
                         + (f" and n_mels = {n_mels}" if n_mels is not None else ""))
    return int(ring.shape[0]), int(ring.shape[1]), R


def stream_logmel_plan(n_channels, ring_len, bank_len, starts, lengths, base, seen, ended, frame_lo, frame_hi, n_fft,
                       hop):
    """The host checks and the workgroup table of stream_logmel (pure: no device needed).  Refuses (ValueError) what
    would not give the offline kernel's bits or would read outside a buffer.  -> None if no channel has a frame due, else
    (starts, lengths, base, frame_lo, frame_hi as int64 arrays, group_first (C + 1) int64 prefix sums of the workgroups
    per channel)."""
    C, R = int(n_channels), int(ring_len)
    hop, half = int(hop), int(n_fft) // 2
    st, ln, bs, sn, lo, hi = (_host_i64(v, C, "stream_logmel") for v in (starts, lengths, base, seen, frame_lo,
                                                                           frame_hi))
    en = np.asarray(ended).astype(bool).reshape(-1)
    if en.shape[0] != C:
        raise ValueError(f"stream_logmel: {en.shape[0]} `ended` flags for {C} channels")
    act = hi > lo
    if not act.any():
        return None
    if (lo[act] < 0).any() or (lo[act] & 1).any() or (hi[act] - lo[act] > R).any():
        raise ValueError("stream_logmel: a frame range must start at an even frame >= 0 and hold at most R frames")
    if (st[act] < 0).any() or (ln[act] < 1).any() or (st[act] + ln[act] > int(bank_len)).any() or \
            (ln[act] >= 2 ** 31 - 2 * half - hop).any() or (bs[act] < 0).any() or (bs[act] + ln[act] != sn[act]).any():
        raise ValueError("stream_logmel: a channel's buffer must lie inside the bank and end at the samples seen so far")
    # every position read lies in [base, seen): the first frame's left edge (the reflection at the stream's start is of
    # positions >= 0, so base must be 0 there), the last frame's right edge unless the stream has ended
    first_pos = lo * hop - half
    if (bs[act] > np.maximum(first_pos[act], 0)).any() or ((first_pos[act] < 0) & (sn[act] <= half)).any():
        raise ValueError("stream_logmel: the buffer starts behind the first sample a frame reads")
    opn, end = act & ~en, act & en
    if (((hi[opn] - lo[opn]) & 1) != 0).any() or ((hi[opn] - 1) * hop + half - 1 >= sn[opn]).any():
        raise ValueError("stream_logmel: an open stream emits whole frame pairs whose samples have all arrived")
    if (hi[end] > 1 + sn[end] // hop).any() or (sn[end] <= half).any() or \
            (bs[end] > np.maximum(sn[end] - half - 1, 0)).any():
        raise ValueError("stream_logmel: an ended stream has 1 + seen // hop frames, needs seen > n_fft / 2 and its "
                         "buffer must hold the samples the end reflection reads")
    pairs = -(-(hi - lo) // 2)
    groups = np.where(act, -(-pairs // STREAM_PAIRS_PER_GROUP), 0)
    return st, ln, bs, lo, hi, np.concatenate([[0], np.cumsum(groups)]).astype(np.int64)


def stream_logmel(bank, starts, lengths, base, seen, ended, frame_lo, frame_hi, ring, fs=16000, n_fft=1024,
                  win_len=1024, hop=512, n_mels=64):
    """The new log-mel frames of many live channels in ONE launch (grafp_stream_logmel_f32).
    bank: flat f32 device buffer; channel c's samples are bank[starts[c] : starts[c] + lengths[c]] -- what the caller
    carried over from earlier chunks, then the new chunk -- and the first of them is sample base[c] of the stream, of
    which seen[c] = base[c] + lengths[c] samples have arrived; ended[c]: no more will.  Frames [frame_lo[c], frame_hi[c])
    are written to ring[c, :, f & (R - 1)] (ring: (C, n_mels, R) f32, R a power of two); an empty range does nothing
    for that channel.  The per-channel tables are HOST integers (sequences or arrays).
    The frames are bit-equal to ops.logmel(whole stream)[:, f].  That needs what stream_logmel_plan checks on the host:
    frame_lo even (two frames share one transform), every sample a frame reads inside the buffer, an even number of
    frames while the stream is open, and, once it has ended, no frame beyond 1 + seen // hop.  Only n_fft == 1024 and
    n_mels <= 64 (the model's configuration); anything else is a ValueError.
    -> the number of workgroups launched (0: nothing was due, nothing launched)."""
    _require_gpu(bank, ring)
    if int(n_fft) != 1024 or not 1 <= int(n_mels) <= 64:
        raise ValueError(f"stream_logmel: only n_fft == 1024 and n_mels <= 64 are supported, not n_fft={n_fft}, "
                         f"n_mels={n_mels}")
    C, _, R = _check_ring("stream_logmel", ring, n_mels)
    if bank.dim() != 1 or bank.dtype != torch.float32 or not bank.is_contiguous() or bank.device != ring.device:
        raise ValueError("stream_logmel: the bank must be a flat contiguous f32 buffer on the ring's device")
    plan_ = stream_logmel_plan(C, R, bank.numel(), starts, lengths, base, seen, ended, frame_lo, frame_hi, n_fft, hop)
    if plan_ is None:
        return 0
    st, ln, bs, lo, hi, first = plan_
    n_groups = int(first[-1])
    plan = _mel_plan(ring.device, fs, n_fft, win_len, n_mels)
    # one upload: the four int64 tables, then the two int32 ones (viewed in the same buffer)
    tab = np.concatenate([st, bs, lo, hi, np.zeros(C + 1, np.int64)])
    i32 = tab[4 * C:].view(np.int32)
    i32[:C] = ln
    i32[C:2 * C + 1] = first
    d = torch.from_numpy(tab).to(ring.device)
    d32 = d[4 * C:].view(torch.int32)
    with _timed("stream_logmel", (C, n_groups)):
        check(lib.grafp_stream_logmel_f32(_p(bank), _p(d[0:C]), _p(d32[0:C]), _p(d[C:2 * C]), _p(d[2 * C:3 * C]),
                                          _p(d[3 * C:4 * C]), _p(d32[C:2 * C + 1]), C, n_groups, int(n_fft), int(hop),
                                          int(n_mels), R, _p(plan.window), _p(plan.twiddle), _p(plan.fb),
                                          _p(plan.band_lo), _p(plan.band_hi), _p(ring), _stream()), "stream_logmel")
    return n_groups


def stream_segments(ring, seg_lo, seg_hi, size, step):
    """The new segments of many live channels in ONE launch (grafp_stream_segments_f32).  ring (C, n_mels, R) as
    stream_logmel fills it; segments [seg_lo[c], seg_hi[c]) of channel c (host integers) are frames
    [s * step, s * step + size) read through the ring.  -> (sum(seg_hi - seg_lo), n_mels, size) f32, channel by channel,
    segments ascending: the values ops.unfold_segments gives on the whole spectrogram.  The caller vouches that the ring
    still holds those frames (R >= size + the frames written since segment seg_lo[c] started)."""
    _require_gpu(ring)
    C, n_mels, R = _check_ring("stream_segments", ring)
    size, step = int(size), int(step)
    if not (1 <= size <= R and step >= 1):
        raise ValueError(f"stream_segments: size={size} must lie in [1, R={R}] and step={step} be positive")
    lo, hi = _host_i64(seg_lo, C, "stream_segments"), _host_i64(seg_hi, C, "stream_segments")
    cnt = np.maximum(hi - lo, 0)
    if ((lo < 0) & (cnt > 0)).any() or ((cnt - 1) * step + size > R).any():
        raise ValueError("stream_segments: a segment range must be non-negative and fit the ring")
    first = np.concatenate([[0], np.cumsum(cnt)])
    n = int(first[-1])
    seg = torch.empty((n, n_mels, size), dtype=torch.float32, device=ring.device)
    if n == 0:
        return seg
    if n >= 2 ** 31:
        raise ValueError("stream_segments: too many segments for one launch")
    tab = np.concatenate([lo, np.zeros((C + 2) // 2, np.int64)])
    tab[C:].view(np.int32)[:C + 1] = first
    d = torch.from_numpy(tab).to(ring.device)
    with _timed("stream_segments", (C, n)):
        check(lib.grafp_stream_segments_f32(_p(ring), _p(d[0:C]), _p(d[C:].view(torch.int32)), C, n, n_mels, R, size,
                                            step, _p(seg), _stream()), "stream_segments")
    return seg


# ------------------------------------------------------------------------------------------------
# device-side augmentation (modules/transformations.py:25-48)
# ------------------------------------------------------------------------------------------------
def _i32c(t, device):
    return t.detach().to(device=device, dtype=torch.int32).contiguous()


def _host_ints(t):
    """The values of a HOST tensor as an int64 array; None for a device tensor, which is never read back (no
    synchronisation: the augmentation ops stay graph-capturable, and their caller vouches for what lives on the device)."""
    return None if t.is_cuda else t.detach().reshape(-1).to(torch.int64).numpy()


def _bank(name, bank, lens, device, starts=None):
    """(flat f32 buffer, int64 starts, int32 lengths) of a recording bank.  bank: a flat 1-D buffer with `starts`, or a
    2-D (n, Lmax) array whose row r holds recording r in its first lens[r] elements.  Refuses (ValueError) a bank
    without its tables and, where lens / starts are host tensors, a recording that is empty or leaves the bank."""
    if bank.dim() not in (1, 2):
        raise ValueError(f"{name}: the bank must be a flat buffer with `starts` or a padded (n, Lmax) array")
    if bank.dim() == 1 and starts is None:
        raise ValueError(f"{name}: a flat bank needs the `starts` of its recordings")
    n = int(bank.shape[0]) if bank.dim() == 2 else int(starts.numel())
    if n == 0 or int(lens.numel()) != n:
        raise ValueError(f"{name}: {int(lens.numel())} lengths for {n} recordings (at least one, as many of each)")
    ln = _host_ints(lens)
    if bank.dim() == 2:
        st, room = None, int(bank.shape[1])
    else:
        st, room = _host_ints(starts), int(bank.numel())
    if (ln is not None and (ln < 1).any()) or (st is not None and (st < 0).any()):
        raise ValueError(f"{name}: a recording needs a length >= 1 and a start >= 0")
    if (ln is not None or st is not None) and ((0 if st is None else st) + (1 if ln is None else ln) > room).any():
        raise ValueError(f"{name}: a recording ends beyond the bank")
    bank = _f32c(bank)
    lens = _i32c(lens, device)
    if bank.dim() == 2:
        starts = torch.arange(bank.shape[0], device=device, dtype=torch.int64) * bank.shape[1]
        bank = bank.reshape(-1)
    else:
        starts = starts.detach().to(device=device, dtype=torch.int64).contiguous()
    return bank, starts, lens


def _aug_rows(name, x):
    """x as contiguous f32 (B, T) rows, and whether it came as one (T,) signal."""
    if x.dim() not in (1, 2):
        raise ValueError(f"{name}: x must be (B, T) or (T,)")
    return _f32c(x.reshape(1, -1) if x.dim() == 1 else x), x.dim() == 1


def _per_clip(name, what, t, B, below=None, floor=None):
    """A per-clip argument has B entries; the values of a host tensor lie below `below` (indices: a negative one is
    legal, it skips the clip) and at or above `floor` (offsets, which must also fit the kernel's int32)."""
    if int(t.numel()) != B:
        raise ValueError(f"{name}: {int(t.numel())} entries in `{what}` for {B} clips")
    v = None if below is None and floor is None else _host_ints(t)
    if v is not None and below is not None and (v >= below).any():
        raise ValueError(f"{name}: `{what}` must be below the {below} recordings")
    if v is not None and floor is not None and ((v < floor) | (v >= 2 ** 31)).any():
        raise ValueError(f"{name}: `{what}` must be >= {floor} and fit 32 bits")


def ir_convolve(x, ir_bank, ir_len, ir_index=None, ir_start=None):
    """ApplyImpulseResponse for a batch: x (B,T) f32; the impulse responses as a ragged bank (flat buffer + ir_start
    + ir_len) or a padded (n_ir, Lmax) array + ir_len; ir_index (B) recording per signal (< 0: copied unchanged;
    None: recording 0) -> (B,T), the full convolution truncated to T (grafp_ir_convolve_f32).
    Shapes and counts are checked, and so are the values of lens / starts / ir_index where they are HOST tensors
    (ValueError); device tensors are not read back, their caller vouches that they lie inside the bank."""
    _require_gpu(x, ir_bank)
    x2, squeeze = _aug_rows("ir_convolve", x)
    bank, starts, lens = _bank("ir_convolve", ir_bank, ir_len, x2.device, ir_start)
    B, T = x2.shape
    if ir_index is not None:
        _per_clip("ir_convolve", "ir_index", ir_index, B, below=lens.numel())
    out = torch.empty_like(x2)
    idx = None if ir_index is None else _i32c(ir_index, x2.device)   # (locals: a temporary's block could be re-used)
    check(lib.grafp_ir_convolve_f32(_p(x2), T, B, T, _p(bank), _p(starts), lens.numel(), _p(lens), _p(idx), _p(out), T,
                                    _stream()), "ir_convolve")
    return out[0] if squeeze else out


def mix_snr(x, noise_bank, noise_len, noise_index, noise_offset, snr_db, noise_start=None):
    """AddBackgroundNoise for a batch: out = x + rms(x)/10^(snr/20) * n/(rms(n)+1e-8) with n the circular read of
    recording noise_index[b] (ragged bank: flat buffer + noise_start + noise_len, or a padded (n, Lmax) array) from
    noise_offset[b] (any offset >= 0: the kernel reduces it mod the length); noise_index < 0: copied unchanged
    (grafp_mix_snr_f32).  Checked as ir_convolve's arguments are: counts always, values where the tensor is on the host."""
    _require_gpu(x, noise_bank)
    x2, squeeze = _aug_rows("mix_snr", x)
    bank, starts, lens = _bank("mix_snr", noise_bank, noise_len, x2.device, noise_start)
    B, T = x2.shape
    _per_clip("mix_snr", "noise_index", noise_index, B, below=lens.numel())
    _per_clip("mix_snr", "noise_offset", noise_offset, B, floor=0)
    _per_clip("mix_snr", "snr_db", snr_db, B)
    out = torch.empty_like(x2)
    nbytes = lib.grafp_mix_snr_workspace(B, T)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x2.device)
    idx, off = (_i32c(t, x2.device) for t in (noise_index, noise_offset))
    snr = _f32c(snr_db.to(x2.device))
    check(lib.grafp_mix_snr_f32(_p(x2), T, B, T, _p(bank), _p(starts), lens.numel(), _p(lens), _p(idx), _p(off),
                                _p(snr), _p(out), T, _p(ws), nbytes, _stream()), "mix_snr")
    return out[0] if squeeze else out


def resample_filter(orig_fs, new_fs, lowpass_filter_width=6, rolloff=0.99):
    """The polyphase filter of torchaudio.transforms.Resample(orig_fs, new_fs) with its defaults (sinc_interp_hann):
    -> (orig, new, width, taps) with orig / new the rates over their gcd and taps (new, K = 2*width + orig) float32,
    evaluated in float64 and rounded once (what Resample(dtype=None) caches).  Host-side; no device needed."""
    g = math.gcd(int(orig_fs), int(new_fs))
    orig, new = int(orig_fs) // g, int(new_fs) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    k = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = (-np.arange(new, dtype=np.float64)[:, None] / new + k) * base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    scale = base / orig
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / t)
    return orig, new, width, (sinc * window * scale).astype(np.float32)


def resampled_length(n, orig_fs, new_fs):
    """Samples of a length-n track after resample(): ceil(new * n / orig) in integers (rates over their gcd)."""
    g = math.gcd(int(orig_fs), int(new_fs))
    orig, new = int(orig_fs) // g, int(new_fs) // g
    return (new * int(n) + orig - 1) // orig


_RESAMPLE_TAPS = {}


def _resample_taps(orig_fs, new_fs, device):
    """The filter in the kernel's layout [ceil(new/P)][K rounded up to 4][P] (P = GRAFP_RESAMPLE_PHASES), zero padded."""
    key = (int(orig_fs), int(new_fs), str(device))
    if key not in _RESAMPLE_TAPS:
        orig, new, width, taps = resample_filter(orig_fs, new_fs)
        P, K = 10, taps.shape[1]
        n_pb, K4 = -(-new // P), -(-K // 4) * 4
        packed = np.zeros((n_pb * P, K4), dtype=np.float32)
        packed[:new, :K] = taps
        packed = packed.reshape(n_pb, P, K4).transpose(0, 2, 1)
        _RESAMPLE_TAPS[key] = (orig, new, width, K, torch.from_numpy(np.ascontiguousarray(packed)).reshape(-1).to(device))
    return _RESAMPLE_TAPS[key]


def resample(bank, starts, lengths, orig_fs, new_fs, out=None, out_starts=None):
    """torchaudio.transforms.Resample(orig_fs, new_fs) (default filter) of every track of a ragged bank in ONE launch
    (grafp_resample_f32).  bank: flat f32 device buffer; starts / lengths: per-track int64 (device or host).
    -> (out_bank, out_starts, out_lengths), the resampled tracks packed back to back -- or, with `out` and `out_starts`,
    written into `out` at those offsets (the caller sized it).  orig_fs == new_fs: a bit-exact copy."""
    _require_gpu(bank)
    dev = bank.device
    bank = _f32c(bank)
    lens_h = torch.as_tensor(lengths).detach().to("cpu", torch.int64)
    n = lens_h.numel()
    if n == 0:
        raise ValueError("resample: no tracks")
    out_lens_h = torch.tensor([resampled_length(int(v), orig_fs, new_fs) for v in lens_h.tolist()], dtype=torch.int64)
    if out_starts is None:
        out_starts_h = torch.cumsum(out_lens_h, 0) - out_lens_h
        total = int(out_lens_h.sum())
    else:
        out_starts_h = torch.as_tensor(out_starts).detach().to("cpu", torch.int64)
        total = int((out_starts_h + out_lens_h).max())
    out_bank = torch.empty(max(total, 1), dtype=torch.float32, device=dev) if out is None else out
    if out is not None and (out.numel() < total or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.device != dev):
        raise ValueError("resample: `out` must be a contiguous f32 device buffer covering every output track")
    orig, new, width, K, taps = _resample_taps(orig_fs, new_fs, dev)
    in_starts = torch.as_tensor(starts).detach().to(device=dev, dtype=torch.int64).contiguous()
    in_lens, out_starts = lens_h.to(dev), out_starts_h.to(dev)
    for lo in range(0, n, 65535):                 # grid.y holds one track per row
        hi = min(n, lo + 65535)
        check(lib.grafp_resample_f32(_p(bank), _p(in_starts[lo:hi]), _p(in_lens[lo:hi]), _p(out_starts[lo:hi]), hi - lo,
                                     int(lens_h[lo:hi].max()), orig, new, width, K, _p(taps), _p(out_bank), _stream()),
              "resample")
    return out_bank[:total], out_starts, out_lens_h.to(dev)


DRAW_PAIRS_MAX_WINDOW = 40896      # offset_mod that draw_pairs_kernel holds in LDS (DP_MAX_WINDOW of csrc/corpus.hip)


def draw_pairs(bank, track_start, track_len, norm, row_track, uniforms, clip, offset_mod, silence, silent_rows=None):
    """The training crops of NeuralfpDataset.__getitem__ (modules/data.py:70-89) for a whole batch in one launch
    (grafp_draw_pairs_f32): row b tries tracks row_track[b], row_track[b] + 1, ... (mod n) with the uniforms
    uniforms[b, a, 0:3] until both crops are louder than `silence`, and writes them divided by the track's norm.
    -> (x_i, x_j), each (B, clip) f32.  silent_rows: optional int32 device counter of rows whose attempts were all
    silent (the last attempt is written)."""
    _require_gpu(bank, uniforms)
    dev = bank.device
    B, A = int(uniforms.shape[0]), int(uniforms.shape[1])
    if uniforms.dim() != 3 or uniforms.shape[2] != 3:
        raise ValueError("draw_pairs: uniforms must be (B, attempts, 3)")
    if row_track.numel() != B:
        raise ValueError("draw_pairs: one start track per row")
    u = _f32c(uniforms)
    starts = track_start.detach().to(device=dev, dtype=torch.int64).contiguous()
    lens = track_len.detach().to(device=dev, dtype=torch.int64).contiguous()
    nv = _f32c(norm.to(dev))
    rows = _i32c(row_track, dev)
    x_i = torch.empty((B, clip), dtype=torch.float32, device=dev)
    x_j = torch.empty((B, clip), dtype=torch.float32, device=dev)
    if silent_rows is not None and (silent_rows.dtype != torch.int32 or not silent_rows.is_cuda):
        raise ValueError("draw_pairs: silent_rows must be an int32 device tensor")
    check(lib.grafp_draw_pairs_f32(_p(_f32c(bank)), _p(starts), _p(lens), _p(nv), lens.numel(), _p(rows), _p(u), B, A,
                                   int(clip), int(offset_mod), float(silence), _p(x_i), _p(x_j), _p(silent_rows),
                                   _stream()), "draw_pairs")
    return x_i, x_j


# ------------------------------------------------------------------------------------------------
# the per-clip warps of the second training view (csrc/clipwarp.h): speed change and time stretch, what they share
# ------------------------------------------------------------------------------------------------
def _ratio_config(cfg, key):
    """The {key}_prob / {key}_range keys of a configuration, validated: -> (prob, lo, hi), or None when the augmentation
    is off ({key}_prob absent or 0).  {key}_range = [lo, hi] with 0.5 <= lo <= hi <= 2 is required when it is on."""
    prob, rng = cfg.get(f"{key}_prob"), cfg.get(f"{key}_range")
    prob = 0.0 if prob is None else float(prob)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"{key}_prob = {prob} is not a probability")
    if rng is not None:
        if not isinstance(rng, (list, tuple)) or len(rng) != 2:
            raise ValueError(f"{key}_range = {rng!r} must be [lo, hi]")
        lo, hi = float(rng[0]), float(rng[1])
        if not 0.5 <= lo <= hi <= 2.0:
            raise ValueError(f"{key}_range = {rng!r} must satisfy 0.5 <= lo <= hi <= 2")
    if prob == 0.0:
        return None
    if rng is None:
        raise ValueError(f"{key}_prob > 0 needs {key}_range = [lo, hi]")
    return prob, lo, hi


def _warp_args(name, x, ratio, out_len, out):
    """The arguments speed_change and time_stretch share, as the entry points take them: x as f32 rows (B, T_in) with unit
    column stride, ratio as (B,) f32 on x's device, `out` checked or allocated.  -> (x2, r, out, squeeze, B, T_in);
    squeeze: x was 1-D, the caller hands row 0 back."""
    _require_gpu(x, ratio if torch.is_tensor(ratio) else None, out)
    squeeze = x.dim() == 1
    x2 = x.detach().reshape(1, -1) if squeeze else x.detach()
    if x2.dim() != 2:
        raise ValueError(f"{name}: x must be (B, T_in) or (T_in,)")
    if x2.dtype != torch.float32 or x2.stride(1) != 1 or x2.stride(0) < x2.shape[1]:
        x2 = _f32c(x2)
    B, T_in = x2.shape
    if torch.is_tensor(ratio):
        r = _f32c(ratio.to(x2.device)).reshape(-1)
    else:
        r = torch.full((B,), float(ratio), dtype=torch.float32, device=x2.device)
    if r.numel() != B:
        raise ValueError(f"{name}: {r.numel()} ratios for {B} clips")
    if out is None:
        out = torch.empty((B, out_len), dtype=torch.float32, device=x2.device)
    elif (out.dtype != torch.float32 or out.device != x2.device or tuple(out.shape) != (B, out_len)
          or out.stride(1) != 1 or out.stride(0) < out_len):
        raise ValueError(f"{name}: `out` must be a (B, out_len) f32 device tensor with unit column stride")
    return x2, r, out, squeeze, B, T_in


# ------------------------------------------------------------------------------------------------
# speed augmentation (csrc/speed.hip): every clip resampled by its own ratio, read on the device
# ------------------------------------------------------------------------------------------------
def speed_pad(max_ratio):
    """Samples of context in front of (and behind) a clip that is to be played at up to max_ratio: the filter's reach
    6 / c with c = 0.99 * min(1, 1 / max_ratio), rounded up, plus one.  Host-side; no device needed."""
    return math.ceil(6.0 / (0.99 * min(1.0, 1.0 / float(max_ratio)))) + 1


def speed_input_len(out_len, max_ratio):
    """Input samples from which speed_change(x, ratio, out_len, x_offset=speed_pad(max_ratio)) reads no zero padding at
    any ratio <= max_ratio: pad + ceil((out_len - 1) * max_ratio) + 1 + pad."""
    pad = speed_pad(max_ratio)
    return pad + math.ceil((int(out_len) - 1) * float(max_ratio)) + 1 + pad


def speed_config(cfg):
    """The speed keys of a configuration, validated: -> (speed_prob, lo, hi), or None when speed augmentation is off
    (speed_prob absent or 0).  speed_range = [lo, hi] with 0.5 <= lo <= hi <= 2 is required when it is on."""
    return _ratio_config(cfg, "speed")


def speed_change(x, ratio, out_len, x_offset=0, out=None):
    """Every clip of a batch resampled by its own ratio in one launch (grafp_speed_change_f32; the rule is stated in
    csrc/speed.hip): x (B, T_in) or (T_in,) f32, rows may be strided; ratio (B,) f32 device tensor of input samples per
    output sample (clamped to [0.5, 2], NaN = 1; above 1 the clip plays fast and its pitch rises; exactly 1 is a bit
    copy) -- or one number for all clips; output m reads the input at x_offset + m * ratio, zeros outside the row.
    -> (B, out_len) f32 (`out`: written in place, rows may be strided).  The ratios are read on the device: no host
    synchronisation, so the launch can be captured into a HIP graph."""
    out_len = int(out_len)
    x2, r, out, squeeze, B, T_in = _warp_args("speed_change", x, ratio, out_len, out)
    with _timed("speed_change", (B, T_in, out_len)):
        check(lib.grafp_speed_change_f32(_p(x2), x2.stride(0), B, T_in, int(x_offset), _p(r), _p(out), out.stride(0),
                                         out_len, _stream()), "speed_change")
    return out[0] if squeeze else out


# ------------------------------------------------------------------------------------------------
# time-stretch augmentation (csrc/stretch.hip): every clip's tempo changed by its own ratio, pitch kept
# ------------------------------------------------------------------------------------------------
STRETCH_FRAME, STRETCH_HOP, STRETCH_SEARCH = 512, 256, 128      # N, HS and the reach of delta (ST_N, ST_HS, ST_D)


def stretch_frames(out_len):
    """Frames of the rule for out_len outputs: F = ceil(out_len / HS) + 1 (the columns of time_stretch's shifts)."""
    return -(-int(out_len) // STRETCH_HOP) + 1


def stretch_pad(max_ratio):
    """Samples of context in front of a clip that is to be stretched at up to max_ratio: frame 0 starts HS * ratio
    samples before the clip and the search reaches 128 further; ceil(HS * max_ratio) + 128 + 1.  Host-side."""
    return math.ceil(STRETCH_HOP * float(max_ratio)) + STRETCH_SEARCH + 1


def stretch_input_len(out_len, max_ratio):
    """Input samples from which time_stretch(x, ratio, out_len, x_offset=stretch_pad(max_ratio)) reads no zero padding
    at any ratio <= max_ratio.  From the rule: the last frame's last candidate ends at a_{F-1} + 127 + N and its template
    at a_{F-2} + 127 + HS + N (the further of the two below ratio 1), with a_i = pad + floor((i - 1) HS ratio + 0.5)
    rounded up and one sample to spare: pad + max(ceil((F-2) HS r), ceil((F-3) HS r) + HS) + 128 + N + 1."""
    F, r = stretch_frames(out_len), float(max_ratio)
    last = max(math.ceil((F - 2) * STRETCH_HOP * r), math.ceil((F - 3) * STRETCH_HOP * r) + STRETCH_HOP)
    return stretch_pad(r) + last + STRETCH_SEARCH + STRETCH_FRAME + 1


def stretch_config(cfg):
    """The stretch keys of a configuration, validated: -> (stretch_prob, lo, hi), or None when time-stretch augmentation
    is off (stretch_prob absent or 0).  stretch_range = [lo, hi] with 0.5 <= lo <= hi <= 2 is required when it is on."""
    return _ratio_config(cfg, "stretch")


# what the training views need with the two augmentations on or off: the transform and the corpus both take it from here
ViewPlan = collections.namedtuple("ViewPlan", "speed stretch clip speed_pad speed_len stretch_pad pad draw_len on")


def view_plan(cfg):
    """The geometry of the training views, from the speed and stretch keys (both pairs validated): the second view is
    stretched, then sped up (GPUTransformNeuralfp.train_transform), so draw_len samples are drawn per view, time_stretch
    turns them into speed_len and speed_change into clip; the first view's clip starts pad = stretch_pad + speed_pad
    samples into its draw.  speed / stretch: (prob, lo, hi) or None; on: "stretch and speed", "stretch", "speed" or "".
    clip (and with it speed_len and draw_len) is None when both are off and cfg has no 'dur'."""
    speed, stretch = speed_config(cfg), stretch_config(cfg)
    clip = int(cfg["fs"] * cfg["dur"]) if speed or stretch or "dur" in cfg else None
    speed_len = speed_input_len(clip, speed[2]) if speed else clip
    sp, st = speed_pad(speed[2]) if speed else 0, stretch_pad(stretch[2]) if stretch else 0
    draw_len = stretch_input_len(speed_len, stretch[2]) if stretch else speed_len
    on = " and ".join(n for n, c in (("stretch", stretch), ("speed", speed)) if c)
    return ViewPlan(speed, stretch, clip, sp, speed_len, st, st + sp, draw_len, on)


def time_stretch(x, ratio, out_len, x_offset=0, out=None, return_shifts=False):
    """Every clip of a batch time-stretched by its own ratio in one launch, pitch kept (grafp_time_stretch_f32; WSOLA,
    the rule is stated in csrc/stretch.hip): x (B, T_in) or (T_in,) f32, rows may be strided; ratio (B,) f32 device tensor
    of input samples per output sample (clamped to [0.5, 2], NaN = 1; above 1 the clip plays fast; exactly 1 is a bit
    copy) -- or one number for all clips; frame i is taken near input x_offset + (i - 1) * 256 * ratio, zeros outside the
    row.  -> (B, out_len) f32 (`out`: written in place, rows may be strided); with return_shifts=True also the
    (B, stretch_frames(out_len)) int32 shifts delta_i of the frames, which say where the splices are.  The ratios are
    read on the device: no host synchronisation, so the launch can be captured into a HIP graph."""
    out_len = int(out_len)
    x2, r, out, squeeze, B, T_in = _warp_args("time_stretch", x, ratio, out_len, out)
    shifts = torch.empty((B, stretch_frames(out_len)), dtype=torch.int32, device=x2.device) if return_shifts else None
    with _timed("time_stretch", (B, T_in, out_len)):
        check(lib.grafp_time_stretch_f32(_p(x2), x2.stride(0), B, T_in, int(x_offset), _p(r), _p(out), out.stride(0),
                                         out_len, _p(shifts), shifts.stride(0) if return_shifts else 0, _stream()),
              "time_stretch")
    if squeeze:
        out, shifts = out[0], (shifts[0] if return_shifts else None)
    return (out, shifts) if return_shifts else out


# ------------------------------------------------------------------------------------------------
# K2  peak extractor
# ------------------------------------------------------------------------------------------------
_RAMPS = {}


def _ramps(device, H, W):
    key = (str(device), H, W)
    if key not in _RAMPS:
        _RAMPS[key] = (torch.linspace(0, 1, steps=W).to(device), torch.linspace(0, 1, steps=H).to(device))
    return _RAMPS[key]


class _PeakExtract(torch.autograd.Function):
    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, spec, weight, bias, stride_h):
        _require_gpu(spec, weight, bias)
        spec, weight, bias = _f32c(spec), _f32c(weight), _f32c(bias)
        B, H, W = spec.shape
        F, cin, KH, KW = weight.shape
        if cin != 3:
            raise ValueError("peak extractor expects 3 input planes [T-ramp, F-ramp, spectrogram]")
        Ho = (H + 2 * (KH // 2) - KH) // stride_h + 1
        t_ramp, f_ramp = _ramps(spec.device, H, W)
        out = torch.empty((B, F, Ho * W), dtype=torch.float32, device=spec.device)
        with _timed("peak_extract_fwd", (B,)):
            check(lib.grafp_peak_extract_fwd_f32(_p(spec), B, H, W, _p(weight), _p(bias), F, KH, KW, stride_h,
                                                 _p(t_ramp), _p(f_ramp), _p(out), _stream()), "peak_extract_fwd")
        ctx.save_for_backward(spec, out)
        ctx.geom = (B, H, W, F, KH, KW, stride_h)
        return out

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        spec, out = ctx.saved_tensors
        B, H, W, F, KH, KW, stride_h = ctx.geom
        g = _f32c(grad_out)
        dw = torch.empty((F, 3, KH, KW), dtype=torch.float32, device=spec.device)
        db = torch.empty((F,), dtype=torch.float32, device=spec.device)
        t_ramp, f_ramp = _ramps(spec.device, H, W)
        nbytes = lib.grafp_peak_extract_bwd_workspace(B, F, KH, KW)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=spec.device)      # per-workgroup partial sums
        with _timed("peak_extract_bwd", (B,)):
            check(lib.grafp_peak_extract_bwd_f32(_p(spec), B, H, W, F, KH, KW, stride_h, _p(t_ramp), _p(f_ramp),
                                                 _p(out), _p(g), _p(dw), _p(db), _p(ws), nbytes, _stream()),
                  "peak_extract_bwd")
        return None, dw, db, None


def peak_extract(spec, weight, bias, stride_h):
    """(B,H,W) log-mel -> (B,F,Ho*W) node features; differentiable w.r.t. weight and bias."""
    return _PeakExtract.apply(spec, weight, bias, int(stride_h))


# ------------------------------------------------------------------------------------------------
# K3-K5  k-NN graph
# ------------------------------------------------------------------------------------------------
_DT = {torch.float32: 0, torch.bfloat16: 1}


def _act_view(x, layout):
    """Return (tensor, B, C, N, stride_b, stride_c) for an activation in 'bcn' = (B,C,N) or 'cbn' = (C,B,N)
    layout (N contiguous), f32 or bf16, without copying when it already is contiguous."""
    if x.dtype not in _DT:
        x = x.float()
    x = x.contiguous()
    if layout == "bcn":
        B, C, N = x.shape
        return x, B, C, N, C * N, N
    C, B, N = x.shape
    return x, B, C, N, N, B * N


def knn_graph(x, k, normalize=True, layout="bcn", index_dtype=torch.int64, prefilter=None):
    """x (B,C,N) / (B,C,N,1) [layout 'bcn'] or (C,B,N) [layout 'cbn'], f32 or bf16 -> int64 (B,N,k)
    nearest-neighbour indices (ascending distance, ties to the lowest index).  Non-differentiable, as in the
    reference (torch_edge.py:78 `no_grad`).  bf16 inputs are widened exactly; all arithmetic is f32."""
    _require_gpu(x)
    if x.dim() == 4:
        x = x.squeeze(-1)
    x, B, C, N, sb, sc = _act_view(x.detach(), layout)
    idx = torch.empty((B, N, k), dtype=index_dtype, device=x.device)
    if (prefilter is None and switches.knn_split and normalize and index_dtype in (torch.int32, torch.int64)
            and lib.grafp_knn_split_preferred_for(_DT[x.dtype], C, N, k) and x.data_ptr() % 16 == 0):
        # split-bf16 Gram matrix + certified order, exact recomputation of the near-ties (knn_split.hip): the same
        # indices bit for bit, ~2x faster than the exact-f32 MFMA kernel below where the library prefers it (f32
        # inputs: C <= 128; bf16 inputs, whose raw features are exact bf16 operands: every stage).  Its 16-byte loads
        # need an aligned first element (the rows are: N % 128 == 0); a view at another storage offset takes the
        # exact-f32 kernel, whose normalisation pass reads element by element
        knn_graph_split(x, k, layout="raw", index_dtype=index_dtype, _view=(x, B, C, N, sb, sc), _out=idx)
        return idx
    if prefilter is None:
        # Off by default.  Measured on MI355X: on random features the pre-filter path wins at C=64, N=1024 (600 vs
        # 920 us per 512 clips), but on the encoder's own early-block features the neighbours are closer than the bf16
        # rounding margin (third-nearest distance ~0.1 vs a margin of 0.03 on each side), the survivor lists overflow
        # and the exact fallback makes it 5-10x slower than the all-f32 kernel.  Kept for callers with well
        # separated data; results are identical either way.
        prefilter = False
    if prefilter and lib.grafp_knn_pre_supported(C, N, k):
        # bf16 pre-filter + exact f32 rescoring (knn_pre.hip): the same indices, several times faster
        nbytes = lib.grafp_knn_pre_workspace(B, C, N)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
        with _timed("knn_topk", (B, C, N, k)):
            check(lib.grafp_knn_graph_pre(_p(x), _DT[x.dtype], sb, sc, B, C, N, k, int(bool(normalize)), _p(idx),
                                          int(index_dtype == torch.int32), _p(ws), nbytes, _stream()), "knn_graph_pre")
        return idx
    xn = torch.empty((B, C, N), dtype=torch.float32, device=x.device)
    sq = torch.empty((B, N), dtype=torch.float32, device=x.device)
    with _timed("knn_normalize", (B, C, N, k)):
        check(lib.grafp_knn_normalize_strided(_p(x), _DT[x.dtype], sb, sc, B, C, N, int(bool(normalize)), _p(xn),
                                              _p(sq), _stream()), "knn_normalize")
    with _timed("knn_topk", (B, C, N, k)):
        topk = lib.grafp_knn_topk_i32 if index_dtype == torch.int32 else lib.grafp_knn_topk_f32
        check(topk(_p(xn), _p(sq), B, C, N, k, _p(idx), _stream()), "knn_topk")
    return idx


def knn_graph_split(x, k, layout="bcn", index_dtype=torch.int64, return_uncertified=False, _view=None, _out=None):
    """The k-NN graph through grafp_knn_graph_split (see knn_graph): (B, N, k) indices; with return_uncertified also a
    0-d int32 device tensor = the number of queries that were recomputed exactly."""
    if _view is None:
        _require_gpu(x)
        if x.dim() == 4:
            x = x.squeeze(-1)
        x, B, C, N, sb, sc = _act_view(x.detach(), layout)
    else:
        x, B, C, N, sb, sc = _view
    if not lib.grafp_knn_split_supported(C, N, k):
        raise ValueError(f"knn_graph_split: unsupported shape C={C} N={N} k={k}")
    idx = _out if _out is not None else torch.empty((B, N, k), dtype=index_dtype, device=x.device)
    nbytes = lib.grafp_knn_split_workspace_for(_DT[x.dtype], B, C, N)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    unc = torch.zeros((), dtype=torch.int32, device=x.device) if return_uncertified else None
    with _timed("knn_split", (B, C, N, k, x.element_size())):
        check(lib.grafp_knn_graph_split(_p(x), _DT[x.dtype], sb, sc, B, C, N, k, _p(idx),
                                        int(idx.dtype == torch.int32), _p(ws), nbytes, _p(unc), _stream()),
              "knn_graph_split")
    return (idx, unc) if return_uncertified else idx


# ------------------------------------------------------------------------------------------------
# K6-K7  gather + max-relative
# ------------------------------------------------------------------------------------------------
class _MaxRelative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, layout):
        _require_gpu(x, idx)
        x, B, C, N, sb, sc = _act_view(x.detach(), layout)
        idx = (idx if idx.dtype == torch.int32 else idx.to(torch.int64)).contiguous()
        K = idx.shape[-1]
        if tuple(idx.shape) != (B, N, K):
            raise ValueError(f"idx shape {tuple(idx.shape)} does not match activations B={B} N={N}")
        out = torch.empty((B, 2 * C, N) if layout == "bcn" else (2 * C, B, N), dtype=x.dtype, device=x.device)
        o_sb, o_sc = (2 * C * N, N) if layout == "bcn" else (N, B * N)
        ctx.layout, ctx.dims = layout, (B, C, N, tuple(x.shape), x.dtype)
        ctx.from_arg = False
        if switches.mrconv_arg and ctx.needs_input_grad[0]:
            # the launch this very call would take with a record: shape, strides and the alignment of x and out decide
            info = (ctypes.c_int * 8)()
            aligned = x.data_ptr() % (4 * x.element_size()) == 0 and out.data_ptr() % (4 * x.element_size()) == 0
            check(lib.grafp_mrconv_plan(_DT[x.dtype], sb, sc, o_sb, o_sc, B, C, N, K, int(aligned), 0, 1, info), "mrconv_plan")
            ctx.from_arg = info[0] == 3
        if ctx.from_arg:
            # training: record which neighbour won (2 bits per element) -- backward then needs neither x nor the gather
            arg = torch.empty((B, C, N // 4), dtype=torch.uint8, device=x.device)
            with _timed("mrconv_fwd", (B, C, N, K)):
                check(lib.grafp_mrconv_fwd_arg(_p(x), _DT[x.dtype], sb, sc, _p(idx), int(idx.dtype == torch.int32), B, C,
                                               N, K, _p(out), o_sb, o_sc, _p(arg), _stream()), "mrconv_fwd_arg")
            ctx.save_for_backward(arg, idx)
            return out
        fwd = lib.grafp_mrconv_fwd_strided_i32 if idx.dtype == torch.int32 else lib.grafp_mrconv_fwd_strided
        with _timed("mrconv_fwd", (B, C, N, K)):
            check(fwd(_p(x), _DT[x.dtype], sb, sc, _p(idx), B, C, N, K, _p(out), o_sb, o_sc, _stream()), "mrconv_fwd")
        ctx.save_for_backward(x, idx)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, idx = ctx.saved_tensors
        layout = ctx.layout
        B, C, N, shape, dtype = ctx.dims
        K = idx.shape[-1]
        g = grad_out.detach().to(dtype).contiguous()
        g_sb, g_sc = (2 * C * N, N) if layout == "bcn" else (N, B * N)
        sb, sc = (C * N, N) if layout == "bcn" else (N, B * N)
        if ctx.from_arg:
            dx = torch.empty(shape, dtype=dtype, device=g.device)
            with _timed("mrconv_bwd", (B, C, N, K)):
                check(lib.grafp_mrconv_bwd_arg(_p(x), _DT[dtype], _p(idx), int(idx.dtype == torch.int32), _p(g), g_sb,
                                               g_sc, B, C, N, K, _p(dx), sb, sc, _stream()), "mrconv_bwd_arg")
            return dx, None, None
        dx = torch.empty_like(x)
        with _timed("mrconv_bwd", (B, C, N, K)):
            bwd = lib.grafp_mrconv_bwd_strided_i32 if idx.dtype == torch.int32 else lib.grafp_mrconv_bwd_strided
            check(bwd(_p(x), _DT[x.dtype], sb, sc, _p(idx), _p(g), g_sb, g_sc, B, C, N, K, _p(dx), _stream()), "mrconv_bwd")
        return dx, None, None


def max_relative(x, idx, layout="bcn"):
    """x (B,C,N) ['bcn'] or (C,B,N) ['cbn'], idx (B,N,K) -> (B,2C,N) / (2C,B,N): channel 2c = x[c],
    channel 2c+1 = max_k(x[c, idx] - x[c]).  f32 or bf16 in = out dtype (arithmetic in f32)."""
    return _MaxRelative.apply(x, idx, layout)


# ------------------------------------------------------------------------------------------------
# K8/K9 glue  fused [conv bias] + BatchNorm + activation + residual on (C, M) rows
# ------------------------------------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


_BN_SYNC = {}


def _bn_sync(device, C, M):
    """The rendezvous buffer of the single-pass BatchNorm kernels: filled with ones once per (device, stream); every
    call leaves it that way (include/grafp_hip.h, grafp_bn_fwd_1pass).  switches.bn_two_pass selects the two-pass
    kernels (None)."""
    if switches.bn_two_pass:
        return None
    key = (device, _raw_stream(device.index if device.index is not None else _cur_device()))
    buf = _BN_SYNC.get(key)
    need = int(lib.grafp_bn_sync_bytes(C, M))
    if buf is None or buf.numel() * 8 < need:
        buf = torch.full((max(1 << 18, (need + 7) // 8),), -1, dtype=torch.int64, device=device)
        _BN_SYNC[key] = buf
    return buf


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, pre_bias, residual, running_mean, running_var, training, momentum, eps, act,
                slope, groups):
        _require_gpu(x, gamma, beta)
        if x.dtype not in _DT:
            x = x.float()
        x = x.detach().contiguous()
        C = x.shape[0]
        M = x.numel() // C
        res = None if residual is None else residual.detach().to(x.dtype).contiguous()
        g32, b32 = _f32c(gamma), _f32c(beta)
        pb = None if pre_bias is None else _f32c(pre_bias)
        out = torch.empty_like(x)
        mean = torch.empty((C, groups), dtype=torch.float32, device=x.device)
        invstd = torch.empty((C, groups), dtype=torch.float32, device=x.device)
        nbytes = lib.grafp_bn_workspace(C, M)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
        with _timed("bn_fwd", (C, M, x.element_size())):
            check(lib.grafp_bn_fwd_1pass(_p(x), _DT[x.dtype], C, M, groups, _p(pb), _p(g32), _p(b32), _p(res), act,
                                         float(slope), float(eps), float(momentum), int(bool(training)),
                                         _p(running_mean), _p(running_var), _p(out), _p(mean), _p(invstd), _p(ws),
                                         nbytes, _p(_bn_sync(x.device, C, M)), switches.bn_spin_limit, _stream()), "bn_fwd")
        ctx.save_for_backward(x, g32, b32, pb if pb is not None else mean.new_empty(0), mean, invstd)
        ctx.cfg = (C, M, act, float(slope), bool(training), pre_bias is not None, residual is not None, groups)
        return out

    @staticmethod
    def backward(ctx, dz):
        x, g32, b32, pb, mean, invstd = ctx.saved_tensors
        C, M, act, slope, training, has_pb, has_res, groups = ctx.cfg
        dz = dz.detach().to(x.dtype).contiguous()
        dx, dgamma, dbeta, dpb = _bn_bwd(x.view(C, M), dz.view(C, M), C, M, groups, pb if has_pb else None, g32, b32, mean,
                                         invstd, act, slope, training)
        return dx.view(x.shape), dgamma, dbeta, dpb, (dz if has_res else None), None, None, None, None, None, None, None, None


def bn_act(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, pre_bias=None, residual=None,
           act=ACT_NONE, slope=0.0, groups=1):
    """z = act(BatchNorm(x + pre_bias)) + residual over ROWS of x (C, ...): one fused HIP forward (2 passes) and
    backward (2 passes).  x / residual / z share a dtype (f32 or bf16); parameters and statistics are f32.
    running_mean / running_var are updated in place when training.  groups > 1: each row is that many equal
    column segments (the views of a contrastive batch) normalised with their own batch statistics."""
    return _BnAct.apply(x, gamma, beta, pre_bias, residual, running_mean, running_var, training, momentum, eps, act,
                        slope, int(groups))


# ------------------------------------------------------------------------------------------------
# K9  1x1 convolution on (C, M) rows: library GEMMs forward / input-gradient, hand-written weight gradient
# ------------------------------------------------------------------------------------------------
class _Stride2Taps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        x = x.detach().contiguous()
        if x.dtype not in _DT:
            x = x.float()
        N = x.shape[-1]
        rows = x.numel() // N
        n_out = (N - 1) // 2 + 1
        out = torch.empty((3,) + tuple(x.shape[:-1]) + (n_out,), dtype=x.dtype, device=x.device)
        check(lib.grafp_stride2_taps_fwd(_p(x), _DT[x.dtype], rows, N, _p(out), _stream()), "stride2_taps_fwd")
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        shape = ctx.shape
        N = shape[-1]
        g = g.detach().contiguous()
        if g.dtype not in _DT:
            g = g.float()
        dx = torch.empty(shape, dtype=g.dtype, device=g.device)
        check(lib.grafp_stride2_taps_bwd(_p(g), _DT[g.dtype], dx.numel() // N, N, _p(dx), _stream()), "stride2_taps_bwd")
        return dx


def stride2_taps(x):
    """x (..., N) -> (3, ..., n_out): out[t][...][j] = x[...][2j + t - 1] (zero outside), the operand of the 3-tap
    stride-2 node convolution of Downsample as one gather (and one scatter-free transpose in backward)."""
    return _Stride2Taps.apply(x)


_BD_MASKS = {}


def _block_diag_weight(w, groups, dtype=None):
    """(Cout, Cin/g) grouped weight -> dense block-diagonal (Cout, Cin) in `dtype`: for the small groups of the
    max-relative conv one dense GEMM (memory-bound either way) beats a 4-batch GEMM of 32x32 problems.  ONE
    elementwise launch (broadcast product with a cached 0/1 mask, cast included) instead of the fill + one copy per
    block + cast of torch.block_diag."""
    cout, cin_g = w.shape
    dtype = dtype or w.dtype
    key = (groups, w.device, w.dtype)
    mask = _BD_MASKS.get(key)
    if mask is None:
        mask = torch.eye(groups, device=w.device, dtype=w.dtype).reshape(groups, 1, groups, 1)
        _BD_MASKS[key] = mask
    out = torch.empty((groups, cout // groups, groups, cin_g), dtype=dtype, device=w.device)
    torch.mul(w.reshape(groups, cout // groups, 1, cin_g), mask, out=out)
    return out.reshape(cout, groups * cin_g)


def split_planes(x):
    """f32 (..., M) -> (hi, lo) bf16 planes with x ~= hi + lo to 2^-17 (grafp_split_bf16_planes); rows stay rows."""
    _require_gpu(x)
    x = _f32c(x)
    hi = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    lo = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib.grafp_split_bf16_planes(_p(x), x.numel(), _p(hi), _p(lo), _stream()), "split_bf16_planes")
    return hi, lo


def split_gemm_supported(R, K, M):
    # (measured: at stages 0-1 the products are HBM-bound and the split's extra passes cost what its matrix rate saves)
    return bool(switches.f32_split_gemm) and R % 32 == 0 and K % 32 == 0 and M % 128 == 0 and max(R, K) >= 256


def split_gemm_f32(w, x):
    """y = w x for f32 w (R, K) and f32 x (K, M) on the bf16 matrix cores: operands split into bf16 hi / lo planes, y =
    Wh Xh + Wh Xl + Wl Xh with every partial product exact and f32 accumulation (~2^-16 relative; the f32 mode's forward
    and data-gradient products -- grafp_conv1x1_gemm_split_f32)."""
    R, K = w.shape
    M = x.shape[1]
    planes = torch.empty((2 * K, M), dtype=torch.bfloat16, device=x.device)
    x = _f32c(x)
    check(lib.grafp_split_bf16_planes(_p(x), x.numel(), _p(planes[:K]), _p(planes[K:]), _stream()), "split_bf16_planes")
    w = _f32c(w)
    wh = w.to(torch.bfloat16)
    wl = (w - wh.float()).to(torch.bfloat16)
    w3 = torch.cat((wh, wh, wl), dim=1).contiguous()
    y = torch.empty((R, M), dtype=torch.float32, device=x.device)
    with _timed("conv1x1_gemm_split", (R, K, M)):
        check(lib.grafp_conv1x1_gemm_split_f32(_p(w3), _p(planes), R, K, M, _p(y), _stream()), "conv1x1_gemm_split")
    return y


class PreparedWeight:
    """What lowp_weights keeps ready of one convolution's weight (conv._prepared): `lowp` the forward operand, `t` the per-
    group transposed copy or, for the first layer of a residual block, `aug` = [W^T | I]; `owner` that lowp_weights."""
    __slots__ = ("lowp", "t", "aug", "owner")

    def __init__(self, lowp=None, t=None, aug=None, owner=None):
        self.lowp, self.t, self.aug, self.owner = lowp, t, aug, owner


def _forward_operand(w, lowp, dtype):
    """w as (R, -1) rows in `dtype`: the prepared copy `lowp` as it is when its dtype and element count fit, else a cast."""
    R = w.shape[0]
    if lowp is not None and lowp.dtype == dtype and lowp.numel() == w.numel():
        return lowp.detach().reshape(R, -1)
    return w.detach().reshape(R, -1).to(dtype)


class _Conv1x1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, groups, w_lowp=None):
        """x (Cin, M) f32/bf16 rows, w (Cout, Cin/groups) parameter view -> (Cout, M) in x's dtype.
        w_lowp: optional copy of w already in x's dtype (see lowp_weights), saves the per-call cast launch."""
        x = x.detach()
        # w may be the 4-D Conv2d parameter itself (Cout, Cin/g, 1, 1): taking it un-reshaped keeps a view node out of
        # the graph, so the weight gradient returned below is adopted as .grad without a copy
        w2 = w.detach().reshape(w.shape[0], -1)
        batched = groups > 1 and w2.shape[1] >= switches.grouped_bmm_min and x.is_cuda
        if batched:
            # wide groups (stages 2-3: 128 / 256 channels per group): a `groups`-batch GEMM; the dense block-diagonal
            # form spends 4x the flops, which at 1024 x 1024 is no longer free next to the operand traffic
            w3 = w2.to(x.dtype).reshape(groups, w2.shape[0] // groups, w2.shape[1])
            y = torch.bmm(w3, x.reshape(groups, w2.shape[1], -1)).reshape(w2.shape[0], -1)
            ctx.save_for_backward(x, w3)
            ctx.groups, ctx.wshape, ctx.wfull, ctx.batched = groups, tuple(w2.shape), tuple(w.shape), True
            return y
        ctx.batched = False
        if groups > 1:
            dense = _block_diag_weight(w2, groups, x.dtype)
        else:
            dense = _forward_operand(w, w_lowp, x.dtype)
        ctx.split = bool(x.is_cuda and x.dtype == torch.float32 and x.numel() % 8 == 0
                         and split_gemm_supported(dense.shape[0], dense.shape[1], x.shape[1])
                         and split_gemm_supported(dense.shape[1], dense.shape[0], x.shape[1]))
        y = split_gemm_f32(dense, x) if ctx.split else torch.mm(dense, x)
        ctx.save_for_backward(x, dense)
        ctx.groups, ctx.wshape, ctx.wfull = groups, tuple(w2.shape), tuple(w.shape)
        return y

    @staticmethod
    def backward(ctx, g):
        x, dense = ctx.saved_tensors
        groups = ctx.groups
        cout, cin_g = ctx.wshape
        g = g.detach().to(x.dtype).contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            if ctx.batched:
                dx = torch.bmm(dense.transpose(1, 2), g.reshape(groups, cout // groups, -1)).reshape(x.shape)
            elif getattr(ctx, "split", False):
                dx = split_gemm_f32(dense.t().contiguous(), g)
            else:
                dx = torch.mm(dense.t(), g)
        dw = None
        if ctx.needs_input_grad[1]:
            cin, M = x.shape
            if x.dtype == torch.bfloat16 and x.is_cuda:
                dw = torch.empty((cout, cin_g), dtype=torch.float32, device=x.device)
                nbytes = lib.grafp_conv1x1_wgrad_workspace(cout, cin, groups, M)
                ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
                with _timed("conv1x1_wgrad", (cout, cin, groups, M)):
                    check(lib.grafp_conv1x1_wgrad_bf16(_p(g), _p(x), cout, cin, groups, M, _p(dw), _p(ws), nbytes,
                                                       _stream()), "conv1x1_wgrad")
            elif x.dtype == torch.float32 and x.is_cuda and not switches.wgrad_f32_library:
                # f32 step: split-bf16 (hi/lo) x 3 MFMAs inside the same streaming kernel; the library's f32 GEMM
                # runs this tall-K shape ~3.5x slower (switches.wgrad_f32_library selects it)
                dw = torch.empty((cout, cin_g), dtype=torch.float32, device=x.device)
                nbytes = lib.grafp_conv1x1_wgrad_f32_workspace(cout, cin, groups, M)
                ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
                with _timed("conv1x1_wgrad", (cout, cin, groups, M)):
                    check(lib.grafp_conv1x1_wgrad_f32(_p(g), _p(x), cout, cin, groups, M, _p(dw), _p(ws), nbytes,
                                                      _stream()), "conv1x1_wgrad_f32")
            elif groups == 1:
                dw = torch.mm(g, x.t()).float()
            else:
                dw = torch.bmm(g.reshape(groups, cout // groups, M), x.reshape(groups, cin_g, M).transpose(1, 2))
                dw = dw.reshape(cout, cin_g).float()
        return dx, (None if dw is None else dw.reshape(ctx.wfull)), None, None


def autocast_rows(x):
    """x, lowered to the autocast dtype if it is f32 on the GPU under autocast (the rest of a block already flows in it)."""
    lower = torch.is_autocast_enabled() and x.is_cuda and x.dtype == torch.float32
    return x.to(torch.get_autocast_dtype("cuda")) if lower else x


def conv1x1_rows(x, w, groups=1, w_lowp=None):
    """y = W x over (C, M) rows (x contiguous 2-D, lowered by autocast_rows).  The weight gradient of bf16 operands is
    the hand-written split-K kernel (grafp_conv1x1_wgrad_bf16), everything else a plain library GEMM."""
    return _Conv1x1.apply(autocast_rows(x).contiguous(), w, groups, w_lowp)


class lowp_weights:
    """The weights of all 1x1 convolutions prepared for one forward + backward pass: the bf16 copy (forward operand),
    the per-group transposed bf16 copy (data-gradient operand) and, for the first layer of a residual block (conv.
    _shortcut_first), [W^T | I] -- ONE launch of grafp_weights_prepare for every layer whose rows and columns per
    group are multiples of 32, one multi-tensor cast for the rest (the 8-channel stem).  `refresh()` before the layers
    run; conv._prepared (a PreparedWeight) is picked up by encoder/_dense.conv_bn_act.
    The buffers are shared between passes and rewritten by EVERY refresh() (one launch; whether the weights changed
    cannot be seen from the host: fused optimizers and replayed graphs update parameters without touching their version
    counters -- a skip-when-unchanged variant trained on stale copies and was caught by the hit-rate test).  Each refresh
    advances a generation number; a backward pass whose forward pass saw an older generation (another encoder forward,
    possibly after an optimizer step, between the two) raises instead of differentiating against whatever the buffers
    hold by then."""

    def __init__(self, convs):
        self.convs = list(convs)
        self.generation = 0             # advanced by every refresh() of THIS instance (its buffers are its own)
        self._dtype, self._dev = None, None
        self._prepared, self._slow, self._slow_bufs, self._src_ptrs = [], [], [], []
        self._table = self._tile_entry = None

    def _build(self, dtype, dev):
        self._dtype, self._dev = dtype, dev
        self._prepared, self._slow, self._slow_bufs = [PreparedWeight(owner=self) for _ in self.convs], [], []
        rows, tiles, base = [], [], 0
        for c, p in zip(self.convs, self._prepared):
            w = c.weight
            G = c.groups
            Rg, Kg = w.shape[0] // G, w.shape[1]
            if dtype == torch.bfloat16 and Rg % 32 == 0 and Kg % 32 == 0 and w.dtype == torch.float32 and w.is_contiguous():
                p.lowp = lo = torch.empty((w.shape[0], Kg), dtype=dtype, device=dev)
                aug = bool(getattr(c, "_shortcut_first", False)) and G == 1
                ld_t = Rg + Kg if aug else Rg
                wt = torch.zeros((G * Kg, ld_t), dtype=dtype, device=dev)
                if aug:
                    wt[:, Rg:] = torch.eye(Kg, dtype=dtype, device=dev)
                n_t = G * (Rg // 32) * (Kg // 32)
                rows.append([w.data_ptr(), lo.data_ptr(), wt.data_ptr(), Rg, Kg, G, ld_t, base])
                tiles.append(torch.full((n_t,), len(rows) - 1, dtype=torch.int32))
                base += n_t
                p.t, p.aug = (None, wt) if aug else (wt, None)
            elif G == 1:
                p.lowp = torch.empty(w.shape, dtype=dtype, device=dev)
                self._slow.append(c)
                self._slow_bufs.append(p.lowp)
        if rows:
            self._table = torch.tensor(rows, dtype=torch.int64).to(dev)
            self._tile_entry = torch.cat(tiles).to(dev)
        else:
            self._table = self._tile_entry = None

    def refresh(self, dtype):
        ws = [c.weight for c in self.convs]
        if not ws or not ws[0].is_cuda:
            return
        dev = ws[0].device
        stale = (self._dtype != dtype or self._dev != dev or
                 any(c.weight.data_ptr() != ptr for c, ptr in zip(self.convs, self._src_ptrs)))
        if stale:
            self._build(dtype, dev)
            self._src_ptrs = [c.weight.data_ptr() for c in self.convs]
            self._published = False
        self.generation += 1
        with torch.no_grad():
            if self._table is not None:
                check(lib.grafp_weights_prepare(_p(self._table), _p(self._tile_entry), int(self._tile_entry.numel()),
                                                _stream()), "weights_prepare")
            if self._slow:
                torch._foreach_copy_(self._slow_bufs, [c.weight for c in self._slow])
        # the prepared buffers are refreshed IN PLACE: the modules' attribute only changes when the buffers were rebuilt
        # (or cleared) -- re-assigning module attributes of 61 layers on every forward pass was 0.6 ms of host time per step
        if not getattr(self, "_published", False):
            self._publish()
            self._published = True

    def _publish(self):
        for c, p in zip(self.convs, self._prepared):
            c._prepared = p

    def clear(self):
        for c in self.convs:
            c._prepared = None
        self._published = False


# ------------------------------------------------------------------------------------------------
# K9  the 1x1 convolution as the hand-written streaming GEMM (gemm.hip), BatchNorm statistics / normalisation folded in
# ------------------------------------------------------------------------------------------------
def gemm_supported(R, K, groups, M, views=1):
    return bool(lib.grafp_conv1x1_gemm_supported(int(R), int(K), int(groups), int(M), int(views)))


_XL_CHECKED = set()


def _xl_selfcheck(device):
    """Once per process and device, at the first product: the four-wave tile (gemm_xl.h) keeps its accumulators in AGPRs it
    NAMES in asm text.  The build checks the generated code for that contract (Makefile -> tools/check_kernel_regs.py);
    this checks the RESULT: one product the plan sends to that tile, against the same product through the eight-wave tile
    (the identity-affine epilogue form runs on GemmL with the same grid).  A mismatch raises -- there is no fallback."""
    key = (device.type, device.index)
    if key in _XL_CHECKED or torch.cuda.is_current_stream_capturing():
        return
    R, K, M = 256, 512, 4096
    info = (ctypes.c_int * 16)()
    lib.grafp_conv1x1_gemm_plan(R, K, 1, M, 1, info)
    if info[0] != 5:                                   # GM_CFG_XL (gemm.hip): the plan rules moved, the check would be vacuous
        raise RuntimeError(f"libgrafp_hip: the self-check product {R}x{K}x{M} is planned on tile configuration {info[0]}, not "
                           "on the four-wave tile (5): update ops._xl_selfcheck together with gemm_plan")
    g = torch.Generator(device="cpu").manual_seed(0)
    w = (torch.randn(R, K, generator=g) / K ** 0.5).to(device, torch.bfloat16)
    x = torch.randn(K, M, generator=g).to(device, torch.bfloat16)
    tab = torch.tensor([1.0, 0.0], device=device).repeat(R, 1, 1).contiguous()            # (R, views = 1, 2): identity
    y, z = torch.empty((R, M), dtype=torch.bfloat16, device=device), torch.empty((R, M), dtype=torch.bfloat16, device=device)
    ys = torch.empty((R, M), dtype=torch.bfloat16, device=device)
    P = lib.grafp_conv1x1_gemm_partials(R, K, 1, M, 1)
    part = torch.empty((R, 1, max(P, 1), 3), dtype=torch.float32, device=device)
    check(lib.grafp_conv1x1_gemm_bf16(_p(w), _p(x), R, K, 1, M, 1, None, 0, 0.0, _p(y), None, _stream()), "conv1x1_gemm")
    check(lib.grafp_conv1x1_gemm_bf16(_p(w), _p(x), R, K, 1, M, 1, None, 0, 0.0, _p(ys), _p(part), _stream()),
          "conv1x1_gemm")                                                                   # the <STATS> form of training
    check(lib.grafp_conv1x1_gemm_affine_bf16(_p(w), _p(x), R, K, 1, M, 1, _p(tab), 0, 0.0, _p(z), _stream()),
          "conv1x1_gemm_affine")
    ones, zeros = torch.ones(R, device=device), torch.zeros(R, device=device)
    # batch statistics out of the partial sums (training-mode finalize on scratch running statistics)
    mean, invstd, _ = bn_finalize(part, R, K, 1, M, 1, ones, zeros, None, zeros.clone(), ones.clone(), True, 0.1, 1e-5)
    zf = z.float()
    zd = z.double()
    want_mean, want_var = zd.mean(1), zd.var(1, unbiased=False)
    what = None
    for name, yf in (("product", y.float()), ("product with statistics", ys.float())):
        # (the two tiles may add the K chunks in another association: equal up to one bf16 rounding step on a few elements)
        wrong = bool(((yf - zf).abs() > zf.abs() * 2.0 ** -7 + float(zf.abs().max()) * 2.0 ** -15).any())
        if wrong or not bool(torch.isfinite(yf).all()) or float((yf != zf).float().mean()) > 5e-3:
            what = f"{name}: max |diff| {float((yf - zf).abs().max())}"
    if what is None:
        sd = want_var.sqrt()
        if not bool(((mean[:, 0].double() - want_mean).abs() <= 1e-3 * sd + 1e-6).all()) or \
                not bool(((invstd[:, 0].double() * (want_var + 1e-5).sqrt() - 1.0).abs() <= 2e-3).all()):
            what = "statistics epilogue: batch mean / variance of the rounded outputs"
    if what is not None:
        raise RuntimeError(f"libgrafp_hip: the four-wave GEMM tile disagrees with the eight-wave tile on a {R}x{K}x{M} product "
                           f"({what}): this build broke the register contract of gemm_xl.h -- rebuild with the "
                           "pinned toolchain (`make -C grafp_amd/csrc` runs tools/check_kernel_regs.py)")
    _XL_CHECKED.add(key)                               # only a check that PASSED is remembered: a caught error re-raises


def conv1x1_gemm(w, x, groups=1, views=1, pro_tab=None, pro_act=ACT_NONE, pro_slope=0.0, stats=False):
    """y = W f(x): w (R, K/groups) bf16, x (K, M) bf16 rows -> y (R, M) bf16 [, partial statistics (R, views, P, 3) f32].
    pro_tab (K, views, 2) f32: f(x) = act(x * scale + shift) applied to the operand tile on the fly (the BatchNorm +
    activation of the layer that produced x); stats: shifted sums of the rounded outputs for bn_finalize."""
    _require_gpu(w, x)
    if w.dtype != torch.bfloat16 or x.dtype != torch.bfloat16:
        raise TypeError("conv1x1_gemm: bf16 operands")
    _xl_selfcheck(x.device)
    w, x = w.contiguous(), x.contiguous()
    R, K, M = w.shape[0], x.shape[0], x.shape[1]
    if w.shape[1] * groups != K:
        raise ValueError(f"conv1x1_gemm: weight {tuple(w.shape)} x groups {groups} does not match {K} operand rows")
    y = torch.empty((R, M), dtype=torch.bfloat16, device=x.device)
    part = None
    if stats:
        P = lib.grafp_conv1x1_gemm_partials(R, K, groups, M, views)
        part = torch.empty((R, views, max(P, 1), 3), dtype=torch.float32, device=x.device)
    tab = None if pro_tab is None else _f32c(pro_tab)
    with _timed("conv1x1_gemm", (R, K, groups, M)):
        check(lib.grafp_conv1x1_gemm_bf16(_p(w), _p(x), R, K, groups, M, views, _p(tab), int(pro_act), float(pro_slope),
                                          _p(y), _p(part), _stream()), "conv1x1_gemm")
    return (y, part) if stats else y


def conv1x1_gemm_affine(w, x, tab, groups=1, views=1, act=ACT_NONE, slope=0.0):
    """z = act(bf16(W x) * scale + shift): the eval-mode [1x1 conv -> BatchNorm -> activation] chain in one kernel
    (tab (R, views, 2) from bn_finalize(training=False)); bit-identical to conv1x1_gemm + bn_affine."""
    _require_gpu(w, x, tab)
    if w.dtype != torch.bfloat16 or x.dtype != torch.bfloat16:
        raise TypeError("conv1x1_gemm_affine: bf16 operands")
    w, x = w.contiguous(), x.contiguous()
    R, K, M = w.shape[0], x.shape[0], x.shape[1]
    if w.shape[1] * groups != K:
        raise ValueError(f"conv1x1_gemm_affine: weight {tuple(w.shape)} x groups {groups} does not match {K} operand rows")
    z = torch.empty((R, M), dtype=torch.bfloat16, device=x.device)
    tab = _f32c(tab)
    with _timed("conv1x1_gemm", (R, K, groups, M)):
        check(lib.grafp_conv1x1_gemm_affine_bf16(_p(w), _p(x), R, K, groups, M, views, _p(tab), int(act), float(slope),
                                                 _p(z), _stream()), "conv1x1_gemm_affine")
    return z


def conv1x1_gemm_cat(w, x1, x2):
    """y = W [x1; x2] for bf16 rows x1 (K1, M), x2 (K2, M) and w (R, K1 + K2): the concatenation is never materialised."""
    _require_gpu(w, x1, x2)
    if w.dtype != torch.bfloat16 or x1.dtype != torch.bfloat16 or x2.dtype != torch.bfloat16:
        raise TypeError("conv1x1_gemm_cat: bf16 operands")
    w, x1, x2 = w.contiguous(), x1.contiguous(), x2.contiguous()
    R, K1, K2, M = w.shape[0], x1.shape[0], x2.shape[0], x1.shape[1]
    if w.shape[1] != K1 + K2 or x2.shape[1] != M:
        raise ValueError(f"conv1x1_gemm_cat: weight {tuple(w.shape)} vs operands {tuple(x1.shape)} + {tuple(x2.shape)}")
    y = torch.empty((R, M), dtype=torch.bfloat16, device=x1.device)
    with _timed("conv1x1_gemm", (R, K1 + K2, 1, M, K2)):        # K2 rows meet an identity block: moved, not multiplied
        check(lib.grafp_conv1x1_gemm_cat_bf16(_p(w), _p(x1), K1, _p(x2), K2, R, M, _p(y), _stream()), "conv1x1_gemm_cat")
    return y


class ShortcutToken:
    """Hands the shortcut's gradient of a residual block from the backward of its LAST layer (which receives dZ and
    would return it unchanged for the shortcut) to the backward of its FIRST layer (whose data gradient autograd would
    add it to): `x = f(x) + x` then costs no separate accumulate kernel -- see conv1x1_gemm_cat."""
    __slots__ = ("grad",)

    def __init__(self):
        self.grad = None


_EYES = {}


def _eye_bf16(n, device):
    key = (n, str(device))
    if key not in _EYES:
        _EYES[key] = torch.eye(n, dtype=torch.bfloat16, device=device)
    return _EYES[key]


def bn_finalize(part, C, K, groups, M, views, gamma, beta, pre_bias, running_mean, running_var, training, momentum, eps):
    """GEMM partial sums (or, in eval mode, the running statistics) -> (mean (C,views), invstd (C,views),
    tab (C,views,2) = (scale, shift) with z = act(y * scale + shift)); advances the running statistics when training."""
    dev = gamma.device
    mean = torch.empty((C, views), dtype=torch.float32, device=dev)
    invstd = torch.empty((C, views), dtype=torch.float32, device=dev)
    tab = torch.empty((C, views, 2), dtype=torch.float32, device=dev)
    g32, b32 = _f32c(gamma), _f32c(beta)
    pb = None if pre_bias is None else _f32c(pre_bias)
    check(lib.grafp_bn_finalize(_p(part), C, K, groups, M, views, _p(pb), _p(g32), _p(b32), float(eps), float(momentum),
                                int(bool(training)), _p(running_mean), _p(running_var), _p(mean), _p(invstd), _p(tab),
                                _stream()), "bn_finalize")
    return mean, invstd, tab


def bn_finalize_affine(y, part, K, groups, views, gamma, beta, pre_bias, running_mean, running_var, momentum, eps,
                       residual=None, act=ACT_NONE, slope=0.0):
    """bn_finalize (training) + bn_affine in ONE launch (every workgroup combines the partial sums of its row itself):
    -> (z, mean, invstd, tab).  y (C, M) bf16 and `part` from conv1x1_gemm(..., stats=True); 1 <= views <= 4."""
    _require_gpu(y, part)
    C, M = y.shape[0], y.numel() // y.shape[0]
    mean = torch.empty((C, views), dtype=torch.float32, device=y.device)
    invstd = torch.empty((C, views), dtype=torch.float32, device=y.device)
    tab = torch.empty((C, views, 2), dtype=torch.float32, device=y.device)
    g32, b32 = _f32c(gamma), _f32c(beta)
    pb = None if pre_bias is None else _f32c(pre_bias)
    res = None if residual is None else residual.to(torch.bfloat16).contiguous()
    z = torch.empty_like(y)
    with _timed("bn_affine", (C, M, res is not None)):
        check(lib.grafp_bn_finalize_affine_bf16(_p(y), _p(part), C, K, groups, M, views, _p(pb), _p(g32), _p(b32),
                                                float(eps), float(momentum), _p(running_mean), _p(running_var), _p(mean),
                                                _p(invstd), _p(tab), _p(res), int(act), float(slope), _p(z), _stream()),
              "bn_finalize_affine")
    return z, mean, invstd, tab


def bn_affine(y, tab, views=1, residual=None, act=ACT_NONE, slope=0.0):
    """z = act(y * scale + shift) + residual over bf16 (C, M) rows (one read [+ residual], one write)."""
    _require_gpu(y, tab)
    y = y.contiguous()
    C, M = y.shape[0], y.numel() // y.shape[0]
    res = None if residual is None else residual.to(torch.bfloat16).contiguous()
    out = torch.empty_like(y)
    with _timed("bn_affine", (C, M, res is not None)):
        check(lib.grafp_bn_affine_bf16(_p(y), C, M, views, _p(tab), _p(res), int(act), float(slope), _p(out), _stream()),
              "bn_affine")
    return out


def _group_transpose(wl, groups):
    """(R, K/g) grouped weight -> (K, R/g): per group the transposed block, the operand of the data-gradient GEMM."""
    R, Kg = wl.shape
    if groups == 1:
        return wl.t().contiguous()
    return wl.reshape(groups, R // groups, Kg).transpose(1, 2).reshape(groups * Kg, R // groups).contiguous()


def _bn_bwd(y, dz, C, M, views, pb, g32, b32, mean, invstd, act, slope, training):
    """BatchNorm + activation backward on (C, M) rows (grafp_bn_bwd_1pass): -> dy, dgamma, dbeta, dpre_bias."""
    dy = torch.empty_like(y)
    # separate tensors (not views of one buffer): autograd adopts a fresh whole tensor as .grad without a copy
    dgamma = torch.empty((C,), dtype=torch.float32, device=y.device)
    dbeta = torch.empty((C,), dtype=torch.float32, device=y.device)
    # d(pre_bias), written by the kernel: zero under batch statistics, ga*invstd*sum(dy) in eval mode
    dpb = torch.empty((C,), dtype=torch.float32, device=y.device) if pb is not None else None
    nbytes = lib.grafp_bn_workspace(C, M)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=y.device)
    with _timed("bn_bwd", (C, M, y.element_size())):
        check(lib.grafp_bn_bwd_1pass(_p(y), _p(dz), _DT[y.dtype], C, M, views, _p(pb), _p(g32), _p(b32), _p(mean),
                                     _p(invstd), act, slope, int(training), _p(dy), _p(dgamma), _p(dbeta), _p(dpb),
                                     _p(ws), nbytes, _p(_bn_sync(y.device, C, M)), switches.bn_spin_limit, _stream()), "bn_bwd")
    return dy, dgamma, dbeta, dpb


# ---- the reductions of a step's weight gradients, deferred and batched (grafp_wgrad_reduce_multi) ----
_WGRAD_PENDING = None        # None: every weight gradient reduces its own partial sums at once; a list: they queue up


def flush_wgrad_reduce():
    """Reduce every queued weight gradient's partial sums now (one launch per 64 layers).  Called when the block below
    ends and by whoever reads a gradient before that (dist.GradSync packs a bucket while backward is still running)."""
    global _WGRAD_PENDING
    q = _WGRAD_PENDING
    if not q:
        return
    _WGRAD_PENDING = []
    n = len(q)
    parts = (ctypes.c_void_p * n)(*[ws.data_ptr() for ws, _, _, _ in q])
    slices = (ctypes.c_int * n)(*[S for _, S, _, _ in q])
    sizes = (ctypes.c_int64 * n)(*[dw.numel() for _, _, dw, _ in q])
    outs = (ctypes.c_void_p * n)(*[dw.data_ptr() for _, _, dw, _ in q])
    with _timed("conv1x1_wgrad_reduce", (n,)):
        check(lib.grafp_wgrad_reduce_multi(parts, slices, sizes, outs, n, _stream()), "wgrad_reduce_multi")


@contextlib.contextmanager
def defer_wgrad_reduce():
    """Inside the block (a backward pass) the bf16 weight gradients only run their split-K kernels; the partial sums of
    all layers are reduced together when the block ends (or at flush_wgrad_reduce()): ~60 launches fewer per step, the
    same bits.  The returned gradient tensors must not be READ inside the block without a flush.  Which weights produced
    a gradient in the block (_WGRAD_SEEN_IDS) is remembered until the OUTERMOST block ends, across flushes and across
    several backward passes inside it (see _wgrad_plan)."""
    global _WGRAD_PENDING
    if _WGRAD_PENDING is not None:                # nested: the outer block flushes
        yield
        return
    _WGRAD_PENDING = []
    try:
        yield
        flush_wgrad_reduce()
    finally:
        _WGRAD_PENDING = None
        _WGRAD_SEEN_IDS.clear()


# Under data parallelism the parameter gradients live in ONE flat buffer (dist.GradSync) that the bucket all-reduces run on.
# GradSync.open() registers a function here that maps a parameter to its slice of that buffer (or None): the weight
# gradient of a layer is then reduced STRAIGHT into the slice -- autograd takes the tensor over as the parameter's .grad, and
# the bucket's pack step finds it in place (no 50 MB of multi-tensor copies per step at N = 8).
_GRAD_TARGET_OF = None


def _wgrad_bf16(g, x, cout, cin, groups, M, views=1, pro_tab=None, pro_act=ACT_NONE, pro_slope=0.0, tile=-1, may_defer=True,
                out=None):
    """dW = g f(x)^T for bf16 (rows, M) operands -> (cout, cin/groups) f32; pro_tab (cin, views, 2): f = the BatchNorm
    + activation of the layer that produced x, applied on the fly (see conv1x1_gemm).  tile: -1 = the library's rule,
    otherwise that tile configuration (grafp_conv1x1_wgrad_tile_bf16; tests).  out: a contiguous f32 tensor of
    cout * cin / groups elements on x's device to write the gradient into (see _GRAD_TARGET_OF)."""
    if out is not None and out.dtype == torch.float32 and out.is_contiguous() and out.device == x.device \
            and out.numel() == cout * (cin // groups):
        dw = out.view(cout, cin // groups)
    else:
        dw = torch.empty((cout, cin // groups), dtype=torch.float32, device=x.device)
    nbytes = lib.grafp_conv1x1_wgrad_tile_workspace(cout, cin, groups, M, views, int(tile))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    tab = None if pro_tab is None else _f32c(pro_tab)
    # may_defer = False: the gradient is READ inside this backward pass (the weight is not a leaf: Downsample's tap matrix
    # is a slice / permutation of its Conv2d parameter, and autograd scatters the gradient back through those views)
    if _WGRAD_PENDING is not None and may_defer:
        S = ctypes.c_int(0)
        with _timed("conv1x1_wgrad", (cout, cin, groups, M)):
            check(lib.grafp_conv1x1_wgrad_partials_bf16(_p(g), _p(x), cout, cin, groups, M, views, _p(tab), int(pro_act),
                                                        float(pro_slope), int(tile), _p(ws), nbytes, ctypes.byref(S),
                                                        _stream()), "conv1x1_wgrad_partials")
        _WGRAD_PENDING.append((ws, int(S.value), dw, tab))       # (the workspace stays alive until its reduction ran)
        return dw
    with _timed("conv1x1_wgrad", (cout, cin, groups, M)):
        check(lib.grafp_conv1x1_wgrad_tile_bf16(_p(g), _p(x), cout, cin, groups, M, views, _p(tab), int(pro_act),
                                                float(pro_slope), int(tile), _p(dw), _p(ws), nbytes, _stream()),
              "conv1x1_wgrad")
    return dw


conv1x1_wgrad = _wgrad_bf16


# weights that produced a gradient in the running defer_wgrad_reduce() block -- deferred or not, in any backward pass inside
# it; only the end of the outermost block clears it (a flush does not: the weights' .grad may still be about to be summed)
_WGRAD_SEEN_IDS = _WGRAD_DEFERRED_IDS = set()    # (one set: the second is the name it had before, still read by callers)


def _wgrad_plan(w):
    """-> (may_defer, target) for the gradient of w, a leaf parameter (None, a derived weight: autograd reads its gradient).
    may_defer: the gradient may leave backward() with its split-K partial sums unreduced (defer_wgrad_reduce), because
    nothing can READ it before the flush.  That holds for the FIRST gradient of a weight in the running block only: a weight
    shared by two layers gets its gradients summed by autograd in front of AccumulateGrad, and a second backward pass ADDS
    into the .grad the first one left, so every later use flushes what is queued and reduces at once (the set of weights
    seen survives flushes: A B A B cannot defer B twice).  And only while .grad is None (AccumulateGrad then takes the
    tensor over; it would ADD unreduced memory into an existing one: accumulation without zero()), with no tensor hook (it
    receives the gradient inside backward) and no post-accumulate hook but GradSync's (which flushes before it packs a
    bucket).  Everything else reduces immediately: slower, never wrong.  target: only a deferred gradient may be produced in
    place, and only inside a block with a registered _GRAD_TARGET_OF: what that returns for w, otherwise None."""
    in_block = _WGRAD_PENDING is not None
    if w is None:
        return False, None
    if in_block:
        if id(w) in _WGRAD_SEEN_IDS:
            flush_wgrad_reduce()                        # the earlier uses' partial sums: reduced before anyone adds to them
            return False, None
        _WGRAD_SEEN_IDS.add(id(w))
    if w.grad is not None or getattr(w, "_backward_hooks", None) or torch.is_grad_enabled():
        return False, None                              # (create_graph = True keeps grad mode on inside backward)
    hooks = getattr(w, "_post_accumulate_grad_hooks", None)
    if hooks:
        from .dist import GradSync
        if not all(isinstance(getattr(h, "__self__", None), GradSync) for h in hooks.values()):
            return False, None
    return True, (_GRAD_TARGET_OF(w) if in_block and _GRAD_TARGET_OF is not None else None)


def _may_defer(w):
    return _wgrad_plan(w)[0]                            # (the half of the plan that tests and tools ask for)


class _ConvBnAct(torch.autograd.Function):
    """z = act(BatchNorm(W x + bias)) + residual on bf16 (C, M) rows, the bf16 training path of every
    [Conv2d(1x1) -> BatchNorm2d -> activation -> shortcut] chain: ONE hand-written GEMM whose epilogue also yields the
    batch statistics, a per-row finalize, one normalise/activate/add pass.  Backward: BatchNorm backward (single
    pass), data gradient by the same GEMM kernel on the transposed weight, weight gradient by the split-K kernel."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, pre_bias, residual, running_mean, running_var, rest):
        conv_groups, views, training, momentum, eps, act, slope, prepared, links = rest       # as conv_bn_act packs them
        ctx.prepared, ctx.links = prepared, links
        x = x.detach()
        defer, d_in = links.norm_out, links.norm_in          # see LayerLinks; pro: what the producer left for this layer
        ctx.pro = pro = (d_in.tab, int(d_in.act), float(d_in.slope)) if d_in is not None and d_in.tab is not None else None
        ctx.w_param = w if w.is_leaf else None               # (looked at again in backward: see _wgrad_plan)
        # shared prepared buffers in use: remember which preparation this forward pass saw
        shared = prepared.owner is not None and not (prepared.lowp is None and prepared.t is None and prepared.aug is None)
        ctx.lowp_gen = prepared.owner.generation if shared else None
        K, M = x.shape
        R = w.shape[0]
        wl = _forward_operand(w, prepared.lowp, torch.bfloat16)
        g32, b32 = _f32c(gamma), _f32c(beta)
        pb = None if pre_bias is None else _f32c(pre_bias)
        if pro is not None:
            if not training:
                raise RuntimeError("conv_bn_act: a deferred normalisation reached an eval-mode consumer")
            y, part = conv1x1_gemm(wl, x, conv_groups, views, pro_tab=pro[0], pro_act=pro[1], pro_slope=pro[2], stats=True)
        elif training:
            y, part = conv1x1_gemm(wl, x, conv_groups, views, stats=True)
        else:
            y, part = conv1x1_gemm(wl, x, conv_groups, views), None
        res = None if residual is None else residual.detach().to(torch.bfloat16).contiguous()
        if defer is not None:
            if not training or res is not None:
                raise RuntimeError("conv_bn_act: only a training-mode layer without a shortcut can defer its normalisation")
            mean, invstd, tab = bn_finalize(part, R, K, conv_groups, M, views, g32, b32, pb, running_mean, running_var,
                                            True, momentum, eps)
            defer.tab, defer.act, defer.slope = tab, act, slope
            z = y                                            # stands in for act(BN(y)): the consumer normalises on load
        elif training and views <= 4:
            z, mean, invstd, tab = bn_finalize_affine(y, part, K, conv_groups, views, g32, b32, pb, running_mean,
                                                      running_var, momentum, eps, res, act, slope)
        else:
            mean, invstd, tab = bn_finalize(part, R, K, conv_groups, M, views, g32, b32, pb, running_mean, running_var,
                                            training, momentum, eps)
            z = bn_affine(y, tab, views, res, act, slope)
        ctx.save_for_backward(x, wl, y, mean, invstd, g32, b32, pb if pb is not None else mean.new_empty(0))
        ctx.cfg = (R, K, M, conv_groups, views, act, float(slope), bool(training), pb is not None, residual is not None,
                   tuple(w.shape))
        return z

    @staticmethod
    def backward(ctx, dz):
        x, wl, y, mean, invstd, g32, b32, pb = ctx.saved_tensors
        R, K, M, cg, views, act, slope, training, has_pb, has_res, wfull = ctx.cfg
        prepared, tok_in, tok_out = ctx.prepared, ctx.links.shortcut_in, ctx.links.shortcut_out
        if ctx.lowp_gen is not None and ctx.lowp_gen != prepared.owner.generation:
            raise RuntimeError("conv_bn_act backward: the shared low-precision weight buffers were re-prepared (another forward "
                               "of THIS encoder under autocast, possibly after an optimizer step) between this layer's "
                               "forward and backward pass; run backward before the next forward")
        dz = dz.detach().to(torch.bfloat16).contiguous()
        dy, dgamma, dbeta, dpb = _bn_bwd(y, dz, R, M, views, pb if has_pb else None, g32, b32, mean, invstd, act, slope,
                                         training)
        dx = None
        if ctx.needs_input_grad[0]:
            short = tok_in.grad if tok_in is not None else None
            if short is not None:
                # dX = [W^T | I] [dY; dZ_shortcut]: the block input's two gradients in one product, rounded once
                tok_in.grad = None
                w_aug = prepared.aug if prepared.aug is not None else torch.cat((wl.t(), _eye_bf16(K, wl.device)), dim=1)
                dx = conv1x1_gemm_cat(w_aug, dy, short)
            elif prepared.t is not None and prepared.t.is_contiguous():
                dx = conv1x1_gemm(prepared.t, dy, cg, 1)
            else:
                dx = conv1x1_gemm(_group_transpose(wl, cg), dy, cg, 1)
        dw = None
        if ctx.needs_input_grad[1]:
            md, tgt = _wgrad_plan(ctx.w_param)
            if ctx.pro is not None:                        # x is the producer's raw output: the same transform on load
                dw = _wgrad_bf16(dy, x, R, K, cg, M, views, ctx.pro[0], ctx.pro[1], ctx.pro[2], may_defer=md,
                                 out=tgt).reshape(wfull)
            else:
                dw = _wgrad_bf16(dy, x, R, K, cg, M, may_defer=md, out=tgt).reshape(wfull)
        dres = dz if has_res else None
        if has_res and tok_out is not None and tok_out.grad is None:
            tok_out.grad, dres = dz, None                  # the first layer's backward adds it (see above)
        return dx, dw, dgamma, dbeta, dpb, dres, None, None, None      # x, w, gamma, beta, pre_bias, residual + 3 constants


def conv_bn_act_supported(x, cout, conv_groups, views):
    """The fused bf16 path applies to HIP bf16 (K, M) rows whose shape both GEMMs (forward, data gradient) accept."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2):
        return False
    K, M = x.shape
    return conv_bn_act_shape_supported(K, M, cout, conv_groups, views)


def conv_bn_act_shape_supported(K, M, cout, conv_groups, views):
    if not switches.fused_conv_bn:
        return False
    return gemm_supported(cout, K, conv_groups, M, views) and gemm_supported(K, cout, conv_groups, M, 1)


class DeferredNorm:
    """Shared by a layer whose BatchNorm + activation output has exactly ONE consumer, another conv_bn_act (norm_out),
    and that consumer (norm_in): the producer returns its raw convolution output and leaves (scale, shift) here, the consumer
    applies them to the operand tile while it is staged (conv1x1_gemm PRO, and again in its weight gradient).  Saves the
    normalise pass (one read + one write of the widest tensors of a block) where the GEMM is HBM-bound."""

    def __init__(self):
        self.tab, self.act, self.slope = None, ACT_NONE, 0.0


class LayerLinks:
    """The cells a fused layer shares with its neighbours in a residual block, each None or:
      shortcut_in   ShortcutToken: this layer's input IS the block's shortcut, its data gradient takes the token's gradient
      shortcut_out  ShortcutToken: this layer adds the shortcut (`residual` is that input), its backward leaves dZ in the token
      norm_out      DeferredNorm: this layer leaves its BatchNorm + activation to its only consumer (no normalise pass)
      norm_in       DeferredNorm: this layer applies its producer's normalisation on load, in its product and weight gradient"""
    __slots__ = ("shortcut_in", "shortcut_out", "norm_out", "norm_in")

    def __init__(self, shortcut_in=None, shortcut_out=None, norm_out=None, norm_in=None):
        self.shortcut_in, self.shortcut_out, self.norm_out, self.norm_in = shortcut_in, shortcut_out, norm_out, norm_in


_UNPREPARED, _UNLINKED = PreparedWeight(), LayerLinks()      # what a layer without prepared copies / without links sees


def defer_norm_pays(consumer_rows, consumer_operand_rows, M):
    """Measured at 512 and 2048 clip-views (DESIGN.md sections 6 and 12.5): the consumer's output rows <= 128 (stages
    0-1): skipped pass 210-415 us against 0 ... +90 us in the GEMM and +5 ... +120 us in the weight gradient.  256 rows
    (stage 2) at 2048 clip-views (profiles/pro_cost_bench_2048.txt): the product leaves the four-wave tile for the
    eight-wave one (+93 / +182 us), the weight gradient the register-staged tile for the S tile (+104 / +218 us), against
    208 / 416 us of skipped pass: -11 / -18 us per layer, inside the run-to-run spread, so it stays out.  Beyond (stage
    3), the products are matrix-bound and the in-register transform costs more than the pass."""
    return bool(switches.defer_norm) and consumer_rows <= 128


def conv_bn_act(x, w, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, pre_bias=None,
                residual=None, act=ACT_NONE, slope=0.0, conv_groups=1, views=1, prepared=None, links=None):
    """act(BatchNorm(W x + pre_bias)) + residual for bf16 (K, M) rows (see _ConvBnAct).  prepared: the PreparedWeight of
    w (lowp_weights) or None; links: the LayerLinks of a layer inside a residual block or None."""
    prepared, links = prepared or _UNPREPARED, links or _UNLINKED
    if not training and residual is None and switches.fused_eval_affine and not torch.is_grad_enabled():
        # inference without a shortcut (fc1, the grouped conv, ffn1, Downsample): the normalisation rides the GEMM's
        # epilogue -- no y, no second pass, no autograd node
        x = x.detach().contiguous()
        K, M = x.shape
        R = w.shape[0]
        wl = _forward_operand(w, prepared.lowp, torch.bfloat16)
        _, _, tab = bn_finalize(None, R, K, int(conv_groups), M, int(views), gamma, beta, pre_bias, running_mean,
                                running_var, False, momentum, eps)
        return conv1x1_gemm_affine(wl, x, tab, int(conv_groups), int(views), int(act), float(slope))
    if not training and (links.norm_out is not None or links.norm_in is not None):
        raise RuntimeError("conv_bn_act: deferred normalisation is a training-mode construct")
    rest = (int(conv_groups), int(views), bool(training), float(momentum), float(eps), int(act), float(slope), prepared, links)
    return _ConvBnAct.apply(x.contiguous(), w, gamma, beta, pre_bias, residual, running_mean, running_var, rest)


def shortcut_token_supported(x, conv_groups=1):
    """The fused shortcut gradient needs the (K, K + K) x M data-gradient product of the block's first layer."""
    if not switches.shortcut_fusion or conv_groups != 1:
        return False
    K, M = x.shape
    return x.is_cuda and x.dtype == torch.bfloat16 and bool(lib.grafp_conv1x1_gemm_supported(K, 2 * K, 1, M, 1))


# ------------------------------------------------------------------------------------------------
# K12  NT-Xent
# ------------------------------------------------------------------------------------------------
class _NTXent(torch.autograd.Function):
    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, z_i, z_j, tau, zi_all, zj_all, row_begin):
        _require_gpu(z_i, z_j)
        # the kernels read zi_all and zj_all with z_i's width and zi_all's row count: a mismatch would be an out-of-bounds
        # read, so it is refused here, before any launch
        if z_i.dim() != 2 or z_i.shape != z_j.shape:
            raise ValueError(f"ntxent: z_i and z_j must be 2-D of one shape, got {tuple(z_i.shape)} and {tuple(z_j.shape)}")
        if z_j.device != z_i.device:
            raise ValueError(f"ntxent: z_j is on {z_j.device}, z_i (shape {tuple(z_i.shape)}) on {z_i.device}")
        if (zi_all is None) != (zj_all is None):
            raise ValueError(f"ntxent: zi_all and zj_all come together, got only {'zi_all' if zj_all is None else 'zj_all'} "
                             f"(shape {tuple((zi_all if zj_all is None else zj_all).shape)})")
        if zi_all is not None:
            if zi_all.shape != zj_all.shape:
                raise ValueError(f"ntxent: zi_all and zj_all differ in shape: {tuple(zi_all.shape)} and {tuple(zj_all.shape)}")
            if zi_all.dim() != 2 or zi_all.shape[1] != z_i.shape[1]:
                raise ValueError(f"ntxent: zi_all / zj_all of shape {tuple(zi_all.shape)} do not have the width of z_i "
                                 f"{tuple(z_i.shape)}")
            if zi_all.device != z_i.device or zj_all.device != z_i.device:
                raise ValueError(f"ntxent: zi_all (shape {tuple(zi_all.shape)}) on {zi_all.device} and zj_all on "
                                 f"{zj_all.device}, z_i on {z_i.device}")
        n_local, D = z_i.shape
        if zi_all is None:
            zi_all, zj_all, row_begin = z_i, z_j, 0
        zi_all, zj_all = _f32c(zi_all), _f32c(zj_all)
        B_all = zi_all.shape[0]
        npart = lib.grafp_ntxent_num_partials(n_local)
        part = torch.empty((npart,), dtype=torch.float32, device=z_i.device)
        dzi = torch.empty((n_local, D), dtype=torch.float32, device=z_i.device)
        dzj = torch.empty((n_local, D), dtype=torch.float32, device=z_i.device)
        nbytes = lib.grafp_ntxent_workspace(B_all)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=z_i.device)
        with _timed("ntxent", (B_all, n_local, D)):
            check(lib.grafp_ntxent_fwd_bwd_f32(_p(zi_all), _p(zj_all), B_all, D, row_begin, n_local, float(tau),
                                               _p(part), _p(dzi), _p(dzj), _p(ws), nbytes, _stream()), "ntxent")
        ctx.save_for_backward(dzi, dzj)
        return part.sum() / (2.0 * B_all)

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, g):
        dzi, dzj = ctx.saved_tensors
        return g * dzi, g * dzj, None, None, None, None


def ntxent(z_i, z_j, tau, zi_all=None, zj_all=None, row_begin=0):
    """NT-Xent of (z_i, z_j) (each (B,D)).  With zi_all/zj_all (the all-gathered embeddings, no grad) the
    negatives are global: the value is this rank's share of the global mean loss and backward yields the
    gradient of the GLOBAL loss w.r.t. the local rows."""
    return _NTXent.apply(z_i, z_j, float(tau), zi_all, zj_all, int(row_begin))


# ------------------------------------------------------------------------------------------------
# K13  brute-force search
# ------------------------------------------------------------------------------------------------
def row_sqnorm(m):
    _require_gpu(m)
    m = _f32c(m)
    out = torch.empty((m.shape[0],), dtype=torch.float32, device=m.device)
    check(lib.grafp_row_sqnorm_f32(_p(m), m.shape[0], m.shape[1], _p(out), _stream()), "row_sqnorm")
    return out


def rows_to_bf16(db):
    """Round-to-nearest-even bf16 copy of the resident (n,128) f32 database for the pre-filter scan."""
    _require_gpu(db)
    db = _f32c(db)
    out = torch.empty(db.shape, dtype=torch.bfloat16, device=db.device)
    check(lib.grafp_f32_to_bf16(_p(db), db.numel(), _p(out), _stream()), "f32_to_bf16")
    return out


def search_l2(db, db_sqnorm, q, k, id_base=0, max_queries_per_launch=4096, db_bf16=None):
    """Exact squared-L2 top-k of q (nq,128) against the resident db (n,128): (dist f32, ids int64), (nq,k).
    db_bf16 (rows_to_bf16(db)): same results through the bf16 pre-filter scan + exact f32 rescoring."""
    _require_gpu(db, db_sqnorm, q)
    q = _f32c(q)
    n, d = db.shape
    nq = q.shape[0]
    out_d = torch.empty((nq, k), dtype=torch.float32, device=db.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=db.device)
    pre = db_bf16 is not None
    if pre and (db_bf16.dtype != torch.bfloat16 or db_bf16.shape != db.shape or not db_bf16.is_contiguous()):
        raise ValueError("search_l2: db_bf16 must be a contiguous bf16 tensor of db's shape")
    for s in range(0, nq, max_queries_per_launch):
        e = min(nq, s + max_queries_per_launch)
        nbytes = (lib.grafp_knn_search_pre_workspace if pre else lib.grafp_knn_search_workspace)(n, e - s, d, k)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=db.device)
        with _timed("knn_search", (n, e - s, k)):
            if pre:
                check(lib.grafp_knn_search_l2_pre(_p(db), _p(db_bf16), _p(db_sqnorm), n, _p(q[s:e]), e - s, d, k,
                                                  int(id_base), _p(out_d[s:e]), _p(out_i[s:e]), _p(ws), nbytes,
                                                  _stream()), "knn_search_l2_pre")
            else:
                check(lib.grafp_knn_search_l2_f32(_p(db), _p(db_sqnorm), n, _p(q[s:e]), e - s, d, k, int(id_base),
                                                  _p(out_d[s:e]), _p(out_i[s:e]), _p(ws), nbytes, _stream()),
                      "knn_search_l2")
    return out_d, out_i


def _half_rows(name, rows):
    """Refuses anything but the half form's rows: a contiguous torch.bfloat16 tensor of shape (n, 128).  (Host values
    only: holds on any device.)"""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.bfloat16 or rows.dim() != 2 or rows.shape[1] != 128 \
            or not rows.is_contiguous():
        got = f"{rows.dtype} {tuple(rows.shape)}" if isinstance(rows, torch.Tensor) else type(rows).__name__
        raise ValueError(f"{name}: the half form's rows must be a contiguous torch.bfloat16 tensor of shape (n, 128), "
                         f"not {got}")
    return rows


def row_sqnorm_half(rows_bf16):
    """The squared norms of bf16 rows (n, 128): bit for bit row_sqnorm(rows_bf16.float()), without the f32 rows."""
    rows_bf16 = _half_rows("row_sqnorm_half", rows_bf16)
    _require_gpu(rows_bf16)
    out = torch.empty((rows_bf16.shape[0],), dtype=torch.float32, device=rows_bf16.device)
    check(lib.grafp_row_sqnorm_bf16(_p(rows_bf16), rows_bf16.shape[0], 128, _p(out), _stream()), "row_sqnorm_bf16")
    return out


def search_l2_half(db_bf16, db_sqnorm, q, k, id_base=0, max_queries_per_launch=4096):
    """search_l2 against a database held as bf16 rows only (grafp_knn_search_l2_half, 260 bytes a row): bit for bit
    search_l2(U, row_sqnorm(U), q, k, db_bf16=db_bf16) with U = db_bf16.float().  db_sqnorm: row_sqnorm_half(db_bf16).
    Against the f32 rows db_bf16 was rounded from, an inner product moves by at most 2^-8 |q| |x|."""
    db_bf16 = _half_rows("search_l2_half", db_bf16)
    _require_gpu(db_bf16, db_sqnorm, q)
    q = _f32c(q)
    n, d = db_bf16.shape
    nq = q.shape[0]
    out_d = torch.empty((nq, k), dtype=torch.float32, device=db_bf16.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=db_bf16.device)
    for s in range(0, nq, max_queries_per_launch):
        e = min(nq, s + max_queries_per_launch)
        nbytes = lib.grafp_knn_search_pre_workspace(n, e - s, d, k)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=db_bf16.device)
        with _timed("knn_search_half", (n, e - s, k)):
            check(lib.grafp_knn_search_l2_half(_p(db_bf16), _p(db_sqnorm), n, _p(q[s:e]), e - s, d, k, int(id_base),
                                               _p(out_d[s:e]), _p(out_i[s:e]), _p(ws), nbytes, _stream()),
                  "knn_search_l2_half")
    return out_d, out_i


def merge_topk(part_d, part_i):
    """(P,nq,k) partial lists (id < 0 = empty) -> (nq,k) by (distance, id)."""
    _require_gpu(part_d, part_i)
    part_d = _f32c(part_d)
    part_i = part_i.to(torch.int64).contiguous()
    P, nq, k = part_d.shape
    out_d = torch.empty((nq, k), dtype=torch.float32, device=part_d.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=part_d.device)
    with _timed("merge_topk", (P, nq, k)):
        check(lib.grafp_merge_topk(_p(part_d), _p(part_i), P, nq, k, _p(out_d), _p(out_i), _stream()), "merge_topk")
    return out_d, out_i


def _check_items_inside(op, item_row, item_len, n_qrows):
    """Refuses items that do not lie inside the n_qrows query rows (two host synchronisations)."""
    if int((item_row.to(torch.int64) + item_len.to(torch.int64)).max().item()) > n_qrows or \
            int(item_row.min().item()) < 0:
        raise ValueError(f"{op}: an item reaches outside q_rows")


def seq_rerank(index_rows, q_rows, topk_ids, item_row, item_len, top=10, shard=None, max_len=None):
    """Sequence-level rerank of batched segment-search results (eval.py:272-290, one workgroup per item).
    index_rows (n,128) f32 resident database, q_rows (n_q,128) f32, topk_ids (n_q,k) int64, item_row (n_items) int64
    first query row of each item, item_len (n_items) int32 segments per item.
    Returns (ids int64 (n_items, top) best first, -1 padded; scores f32 (n_items, top), -inf padded).
    shard = (row_base, n_total, id_lo, id_hi): index_rows holds global rows [row_base, row_base + len) of an n_total-row
    index and only candidates starting in [id_lo, id_hi) are scored (dist.ShardedFlatL2Index.rerank merges shards).
    max_len: the longest item (segments), an upper bound is fine; the caller then also vouches that every item lies
    inside q_rows (the kernel clamps nothing)."""
    _require_gpu(index_rows, q_rows, topk_ids, item_row, item_len)
    index_rows, q_rows = _f32c(index_rows), _f32c(q_rows)
    topk_ids = topk_ids.to(torch.int64).contiguous()
    item_row = item_row.to(torch.int64).contiguous()
    item_len = item_len.to(torch.int32).contiguous()
    n_items = item_row.shape[0]
    out_i = torch.empty((n_items, top), dtype=torch.int64, device=index_rows.device)
    out_s = torch.empty((n_items, top), dtype=torch.float32, device=index_rows.device)
    if n_items == 0:
        return out_i, out_s
    if max_len is None:
        # convenience path with three host synchronisations (length bound + range check); callers that know the longest
        # sequence pass it (eval.py, dist.py, bench.py do) and stay asynchronous / graph-capturable like the other ops
        max_len = int(item_len.max().item())
        _check_items_inside("seq_rerank", item_row, item_len, q_rows.shape[0])
    max_len = int(max_len)
    with _timed("seq_rerank", (n_items, max_len, topk_ids.shape[1])):
        if shard is None:
            check(lib.grafp_seq_rerank_f32(_p(index_rows), index_rows.shape[0], _p(q_rows), q_rows.shape[0],
                                           _p(topk_ids), topk_ids.shape[1], _p(item_row), _p(item_len), n_items, max_len,
                                           top, _p(out_i), _p(out_s), _stream()), "seq_rerank")
        else:
            row_base, n_total, id_lo, id_hi = (int(v) for v in shard)
            check(lib.grafp_seq_rerank_shard_f32(_p(index_rows), index_rows.shape[0], row_base, n_total, id_lo, id_hi,
                                                 _p(q_rows), q_rows.shape[0], _p(topk_ids), topk_ids.shape[1],
                                                 _p(item_row), _p(item_len), n_items, max_len, top, _p(out_i),
                                                 _p(out_s), _stream()), "seq_rerank_shard")
    return out_i, out_s


IDENTIFY_MAX_LEN, IDENTIFY_MAX_K, IDENTIFY_MAX_KEYS = 256, 32, 8192      # identify.hip's limits


def check_track_table(first, n):
    """Refuses a track table that is not (T + 1) int64 row starts with first[0] = 0, first[T] = n, non-decreasing;
    returns it as a host int64 tensor."""
    f = torch.as_tensor(first).detach().to("cpu", torch.int64).reshape(-1)
    if f.numel() < 2 or int(f[0]) != 0 or int(f[-1]) != int(n) or bool((f[1:] < f[:-1]).any()):
        raise ValueError(f"identify: the track table must run from 0 to n = {int(n)} and never decrease "
                         f"(got {f.numel()} entries{', ' + str(int(f[0])) + ' .. ' + str(int(f[-1])) if f.numel() else ''})")
    return f


def _identify_args(name, n_rows, track_first_row, q_rows, topk_ids, item_row, item_len, top, min_overlap, max_len):
    """The host checks the identify ops share, for a library of n_rows rows -> (n_items, k, top, max_len, min_overlap as
    the int the C entry takes).  Without max_len, and with items, the longest item is read back (the max_len returned)
    and the track table and the item ranges are checked on the host; with it nothing here touches a device.  max_len stays
    None only when there is no item."""
    n_items, k, top = int(item_row.shape[0]), int(topk_ids.shape[1]), int(top)
    # argument checks first (host values only): they hold on any device
    if not 1 <= top <= 64:
        raise ValueError(f"{name}: top={top} not in [1, 64]")
    if not 1 <= k <= IDENTIFY_MAX_K:
        raise ValueError(f"{name}: k={k} hits per segment exceeds {IDENTIFY_MAX_K}")
    if min_overlap is not None and int(min_overlap) < 1:
        raise ValueError(f"{name}: min_overlap must be at least 1 segment")
    if max_len is None and n_items:
        max_len = max(1, int(item_len.max().item()))
        check_track_table(track_first_row, n_rows)
        _check_items_inside(name, item_row, item_len, q_rows.shape[0])
    if max_len is not None and (int(max_len) > IDENTIFY_MAX_LEN or int(max_len) * k > IDENTIFY_MAX_KEYS):
        raise ValueError(f"{name}: items of {int(max_len)} segments with k={k} exceed {IDENTIFY_MAX_LEN} segments "
                         f"or {IDENTIFY_MAX_KEYS} hits per item")
    return (n_items, k, top, None if max_len is None else int(max_len),
            0 if min_overlap is None else int(min_overlap))


def _identify_tensors(dev, track_first_row, topk_ids, item_row, item_len, top, n_outs=4):
    """The track table, the hits and the items in the C entry's dtypes on dev, and the n_outs (n_items, top) results
    (track, offset, score, votes and, for the tempo op, ratio: int32 but score f32), uninitialised."""
    first = torch.as_tensor(track_first_row).detach().to(device=dev, dtype=torch.int64).contiguous()
    topk_ids = topk_ids.to(torch.int64).contiguous()
    item_row = item_row.to(torch.int64).contiguous()
    item_len = item_len.to(torch.int32).contiguous()
    outs = tuple(torch.empty((item_row.shape[0], top), dtype=torch.float32 if j == 2 else torch.int32, device=dev)
                 for j in range(n_outs))
    return first, topk_ids, item_row, item_len, outs


def identify(index_rows, track_first_row, q_rows, topk_ids, item_row, item_len, top=5, min_overlap=None, max_len=None):
    """Track-aware sequence identification (grafp_identify_f32, one workgroup per item): for every item, the `top`
    library tracks it most likely is, with the alignment inside each.
    index_rows (n,128) f32 resident library, track_first_row (T+1) int64 (track t = rows [first[t], first[t+1])),
    q_rows (n_q,128) f32, topk_ids (n_q,k) int64 (-1: no hit), item_row (n_items) int64 first query row of each item,
    item_len (n_items) int32 segments per item.  min_overlap: segments of the query that must lie inside the track
    (None: the whole item, unless the track is shorter).
    Returns (track int32, offset int32 in segments from the track's first row, score f32, votes int32), each
    (n_items, top), best first, padded with -1 / INT_MIN / -inf / 0.
    max_len: the longest item, an upper bound is fine; the caller then vouches for the ranges (the item rows inside
    q_rows, the track table well formed) and the call stays asynchronous and capturable.  Without it the op checks them
    on the host."""
    n_items, k, top, max_len, min_overlap = _identify_args("identify", index_rows.shape[0], track_first_row, q_rows,
                                                           topk_ids, item_row, item_len, top, min_overlap, max_len)
    _require_gpu(index_rows, q_rows, topk_ids, item_row, item_len)
    index_rows, q_rows = _f32c(index_rows), _f32c(q_rows)
    first, topk_ids, item_row, item_len, outs = _identify_tensors(index_rows.device, track_first_row, topk_ids,
                                                                  item_row, item_len, top)
    if n_items == 0:
        return outs
    with _timed("identify", (n_items, max_len, k)):
        check(lib.grafp_identify_f32(_p(index_rows), index_rows.shape[0], _p(first), first.numel() - 1, _p(q_rows),
                                     q_rows.shape[0], _p(topk_ids), k, _p(item_row), _p(item_len), n_items, max_len,
                                     top, min_overlap, *(_p(o) for o in outs), _stream()), "identify")
    return outs


def identify_half(index_rows_bf16, track_first_row, q_rows, topk_ids, item_row, item_len, top=5, min_overlap=None,
                  max_len=None):
    """ops.identify against a library held as bf16 rows (grafp_identify_half_f32): index_rows_bf16 (n, 128) contiguous
    torch.bfloat16, and every output is bit for bit what ops.identify returns on index_rows_bf16.float().  The other
    arguments, max_len's promise and the results as for ops.identify.  Against the f32 rows the bf16 rows were rounded
    from, a score moves by at most 2^-8 max||q|| max||x||."""
    index_rows_bf16 = _half_rows("identify_half", index_rows_bf16)
    n_items, k, top, max_len, min_overlap = _identify_args("identify_half", index_rows_bf16.shape[0], track_first_row,
                                                           q_rows, topk_ids, item_row, item_len, top, min_overlap,
                                                           max_len)
    _require_gpu(index_rows_bf16, q_rows, topk_ids, item_row, item_len)
    q_rows = _f32c(q_rows)
    first, topk_ids, item_row, item_len, outs = _identify_tensors(index_rows_bf16.device, track_first_row, topk_ids,
                                                                  item_row, item_len, top)
    if n_items == 0:
        return outs
    with _timed("identify_half", (n_items, max_len, k)):
        check(lib.grafp_identify_half_f32(_p(index_rows_bf16), index_rows_bf16.shape[0], _p(first), first.numel() - 1,
                                          _p(q_rows), q_rows.shape[0], _p(topk_ids), k, _p(item_row), _p(item_len),
                                          n_items, max_len, top, min_overlap, *(_p(o) for o in outs), _stream()),
              "identify_half")
    return outs


IDENTIFY_MAX_STRIDE = 32                                            # identify_thin.hip's largest row stride


def identify_thin(index_rows, track_first_row, q_rows, topk_ids, item_row, item_len, row_stride, top=5,
                  min_overlap=None, max_len=None):
    """ops.identify against a library that keeps every row_stride-th row of each track (grafp_identify_thin_f32):
    row j of track t is that track's dense segment j * D (D = row_stride in [1, 32]), a track of S dense segments has
    ceil(S / D) rows, and track_first_row counts kept rows.  The query rows stay dense.
    A hit (s, r) names the track t holding r and the fine alignment a = r * D - s; the pairs of (t, a) are the query
    rows s with (a + s) mod D == 0 whose row (a + s) / D lies inside t, o of them; the candidate is eligible iff
    o >= 1 and o >= min(max(1, need // D), rows of t) with need = min_overlap (None: the item's length), and scores the
    mean dot product over its pairs in ops.identify's arithmetic order.  offset = a - first[t] * D: dense segments from
    the track's start, as ops.identify reports it.  Everything else (arguments, ranking, padding, max_len) as for
    ops.identify, which this equals bit for bit at row_stride = 1."""
    D = int(row_stride)
    # argument checks first (host values only): they hold on any device
    if not 1 <= D <= IDENTIFY_MAX_STRIDE:
        raise ValueError(f"identify_thin: row_stride={D} not in [1, {IDENTIFY_MAX_STRIDE}]")
    if int(index_rows.shape[0]) * D + IDENTIFY_MAX_LEN - 1 >= 1 << 32:
        raise ValueError(f"identify_thin: {int(index_rows.shape[0])} rows at row_stride={D} reach past the 2^32 fine "
                         "positions an alignment key holds")
    n_items, k, top, max_len, min_overlap = _identify_args("identify_thin", index_rows.shape[0], track_first_row, q_rows,
                                                           topk_ids, item_row, item_len, top, min_overlap, max_len)
    _require_gpu(index_rows, q_rows, topk_ids, item_row, item_len)
    index_rows, q_rows = _f32c(index_rows), _f32c(q_rows)
    first, topk_ids, item_row, item_len, outs = _identify_tensors(index_rows.device, track_first_row, topk_ids,
                                                                  item_row, item_len, top)
    if n_items == 0:
        return outs
    with _timed("identify_thin", (n_items, max_len, k, D)):
        check(lib.grafp_identify_thin_f32(_p(index_rows), index_rows.shape[0], _p(first), first.numel() - 1, D,
                                          _p(q_rows), q_rows.shape[0], _p(topk_ids), k, _p(item_row), _p(item_len),
                                          n_items, max_len, top, min_overlap, *(_p(o) for o in outs), _stream()),
              "identify_thin")
    return outs


IDENTIFY_MAX_QUERY_STRIDE = 32                                           # identify_stride.hip's largest query stride


def identify_stride(index_rows, track_first_row, q_rows, topk_ids, item_row, item_len, query_stride, top=5,
                    min_overlap=None, max_len=None):
    """ops.identify for items whose rows are every query_stride-th segment of the recording
    (grafp_identify_stride_f32): item row s is the recording's segment s * Q (Q = query_stride in [1, 32]), so it sits
    s * Q library rows after item row 0.  The library is dense; item_len, max_len and min_overlap count kept rows.
    A hit (s, r) names the track t holding r and the alignment a = r - s * Q; the pairs of (t, a) are the item rows s
    with a + s * Q inside t, o of them; the candidate is eligible iff o >= 1 and o >= min(need, max(1, rows of t // Q))
    with need = min_overlap (None: the item's length), and scores the mean dot product over its pairs in ops.identify's
    arithmetic order.  offset = a - first[t]: where the item's first row sits in the track, in dense segments.
    Everything else (arguments, ranking, padding, max_len) as for ops.identify, which this equals bit for bit at
    query_stride = 1; at 2 it equals the first four outputs of ops.identify_tempo at ratio_num = [512]."""
    Q = int(query_stride)
    # argument checks first (host values only): they hold on any device
    if not 1 <= Q <= IDENTIFY_MAX_QUERY_STRIDE:
        raise ValueError(f"identify_stride: query_stride={Q} not in [1, {IDENTIFY_MAX_QUERY_STRIDE}]")
    if int(index_rows.shape[0]) + (IDENTIFY_MAX_LEN - 1) * Q >= 1 << 32:
        raise ValueError(f"identify_stride: {int(index_rows.shape[0])} rows at query_stride={Q} reach past the 2^32 "
                         "alignments a key holds")
    n_items, k, top, max_len, min_overlap = _identify_args("identify_stride", index_rows.shape[0], track_first_row,
                                                           q_rows, topk_ids, item_row, item_len, top, min_overlap, max_len)
    _require_gpu(index_rows, q_rows, topk_ids, item_row, item_len)
    index_rows, q_rows = _f32c(index_rows), _f32c(q_rows)
    first, topk_ids, item_row, item_len, outs = _identify_tensors(index_rows.device, track_first_row, topk_ids,
                                                                  item_row, item_len, top)
    if n_items == 0:
        return outs
    with _timed("identify_stride", (n_items, max_len, k, Q)):
        check(lib.grafp_identify_stride_f32(_p(index_rows), index_rows.shape[0], _p(first), first.numel() - 1, Q,
                                            _p(q_rows), q_rows.shape[0], _p(topk_ids), k, _p(item_row), _p(item_len),
                                            n_items, max_len, top, min_overlap, *(_p(o) for o in outs), _stream()),
              "identify_stride")
    return outs


IDENTIFY_TEMPO_MAX_RATIOS = 64                                           # identify_tempo.hip's ratios per call
IDENTIFY_TEMPO_MIN, IDENTIFY_TEMPO_MAX, IDENTIFY_TEMPO_DEN = 128, 512, 256   # a ratio is num / 256


def identify_tempo(index_rows, track_first_row, q_rows, topk_ids, item_row, item_len, ratio_num, top=5,
                   min_overlap=None, max_len=None):
    """ops.identify for recordings that play faster or slower than the catalogue (grafp_identify_tempo_f32: one
    workgroup per item and ratio, then one per item that merges the ratios' lists).  ratio_num: 1 to 64 strictly
    ascending integers in [128, 512] (host values), each standing for num / 256 track seconds per recording second.
    At ratio num query row s sits w(s) = (s * num + 128) >> 8 library rows after query row 0.  A hit (s, r) names the
    track t holding r and the alignment a = r - w(s); the pairs of (t, a, num) are the query rows s with a + w(s) inside
    t, o of them; the candidate is eligible iff o >= 1 and o >= min(need, max(1, rows of t * 256 // num)) with need =
    min_overlap (None: the item's length), and scores the mean dot product over its pairs in ops.identify's arithmetic
    order.  Per track the best candidate: highest score, then the ratio nearer to 1 (smaller |num - 256|, then smaller
    num), then the smaller a.
    Returns (track, offset, score, votes, ratio int32 = num), each (n_items, top), padded with -1 / INT_MIN / -inf / 0 /
    0; offset = a - first[t] is where the item's first row sits in the track.  Everything else (arguments, ranking,
    max_len) as for ops.identify, whose four outputs this equals bit for bit at ratio_num = [256]."""
    n_items, k, top, max_len, min_overlap = _identify_args("identify_tempo", index_rows.shape[0], track_first_row,
                                                           q_rows, topk_ids, item_row, item_len, top, min_overlap, max_len)
    ratios = _tempo_ratio_list("identify_tempo", ratio_num)
    if int(index_rows.shape[0]) + 2 * IDENTIFY_MAX_LEN - 1 >= 1 << 32:
        raise ValueError(f"identify_tempo: {int(index_rows.shape[0])} rows reach past the 2^32 alignments a key holds")
    _require_gpu(index_rows, q_rows, topk_ids, item_row, item_len)
    index_rows, q_rows = _f32c(index_rows), _f32c(q_rows)
    dev = index_rows.device
    first, topk_ids, item_row, item_len, outs = _identify_tensors(dev, track_first_row, topk_ids, item_row, item_len,
                                                                  top, n_outs=5)
    if n_items == 0:
        return outs
    nums = (ctypes.c_int32 * len(ratios))(*ratios)                       # read by the entry before it returns
    ws = torch.empty(lib.grafp_identify_tempo_workspace(n_items, len(ratios), top), dtype=torch.uint8, device=dev)
    with _timed("identify_tempo", (n_items, max_len, k, len(ratios))):
        check(lib.grafp_identify_tempo_f32(_p(index_rows), index_rows.shape[0], _p(first), first.numel() - 1,
                                           _p(q_rows), q_rows.shape[0], _p(topk_ids), k, _p(item_row), _p(item_len),
                                           n_items, max_len, top, min_overlap, ctypes.cast(nums, ctypes.c_void_p),
                                           len(ratios), _p(ws), *(_p(o) for o in outs), _stream()), "identify_tempo")
    return outs


def tempo_work_table(n_ratios, item_ratio_lo, item_ratio_cnt, name="identify_tempo_items"):
    """The work table of ops.identify_tempo_items over a grid of n_ratios ratios: item i is searched over the ratios
    [lo_i, lo_i + cnt_i) -> (table, n_work, max_cnt): table is one int32 host array holding the n_work = sum(cnt)
    entries (item, ratio index), ordered by item and then by ratio, followed by the exclusive scan of cnt
    (n_items + 1 values).  Refuses, naming the first such item, a window with cnt < 1, lo < 0 or lo + cnt > n_ratios."""
    lo = np.asarray(item_ratio_lo, np.int64).reshape(-1)
    cnt = np.asarray(item_ratio_cnt, np.int64).reshape(-1)
    if lo.shape != cnt.shape:
        raise ValueError(f"{name}: {lo.size} item_ratio_lo for {cnt.size} item_ratio_cnt")
    bad = np.nonzero((cnt < 1) | (lo < 0) | (lo + cnt > int(n_ratios)))[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"{name}: item {i}'s ratio window lo={int(lo[i])} cnt={int(cnt[i])} does not lie inside the "
                         f"{int(n_ratios)} ratios of the call (1 <= cnt, 0 <= lo, lo + cnt <= {int(n_ratios)})")
    scan = np.concatenate([[0], np.cumsum(cnt)])
    n_work = int(scan[-1])
    item = np.repeat(np.arange(lo.size, dtype=np.int64), cnt)
    ratio = np.arange(n_work, dtype=np.int64) - scan[item] + lo[item]
    table = np.concatenate([np.stack([item, ratio], axis=1).reshape(-1), scan]).astype(np.int32)
    return table, n_work, int(cnt.max(initial=0))


def identify_tempo_items(index_rows, track_first_row, q_rows, topk_ids, item_row, item_len, ratio_num, item_ratio_lo,
                         item_ratio_cnt, top=5, min_overlap=None, max_len=None):
    """ops.identify_tempo with a ratio window per item (grafp_identify_tempo_items_f32): ratio_num is the call's
    ascending grid of R <= 64 ratios, and item i is identified over ratio_num[lo_i : lo_i + cnt_i] only, with the host
    arrays item_ratio_lo, item_ratio_cnt (n_items each; 1 <= cnt, 0 <= lo, lo + cnt <= R; anything else is a ValueError
    that names the item).  Row i of the five outputs equals, bit for bit, row 0 of ops.identify_tempo called with item i
    alone and that sub-list of ratios -- the tie rule (the ratio nearer to 1, then the smaller num, then the smaller
    alignment) applies among the item's own ratios -- and with every cnt = R the outputs are ops.identify_tempo's.
    One workgroup per item and ratio OF ITS WINDOW (sum(cnt) of them, listed in a small int32 work table that is built
    here and uploaded), then one per item that merges its lists; no host synchronisation.  Everything else (arguments,
    outputs, padding, max_len) as for ops.identify_tempo."""
    name = "identify_tempo_items"
    n_items, k, top, max_len, min_overlap = _identify_args(name, index_rows.shape[0], track_first_row, q_rows, topk_ids,
                                                           item_row, item_len, top, min_overlap, max_len)
    ratios = _tempo_ratio_list(name, ratio_num)
    if len(np.asarray(item_ratio_cnt).reshape(-1)) != n_items or len(np.asarray(item_ratio_lo).reshape(-1)) != n_items:
        raise ValueError(f"{name}: item_ratio_lo and item_ratio_cnt must hold one value per item ({n_items})")
    table, n_work, max_cnt = tempo_work_table(len(ratios), item_ratio_lo, item_ratio_cnt, name)
    if int(index_rows.shape[0]) + 2 * IDENTIFY_MAX_LEN - 1 >= 1 << 32:
        raise ValueError(f"{name}: {int(index_rows.shape[0])} rows reach past the 2^32 alignments a key holds")
    _require_gpu(index_rows, q_rows, topk_ids, item_row, item_len)
    index_rows, q_rows = _f32c(index_rows), _f32c(q_rows)
    dev = index_rows.device
    first, topk_ids, item_row, item_len, outs = _identify_tensors(dev, track_first_row, topk_ids, item_row, item_len,
                                                                  top, n_outs=5)
    if n_items == 0:
        return outs
    nums = (ctypes.c_int32 * len(ratios))(*ratios)                       # read by the entry before it returns
    table = torch.from_numpy(table).to(dev)                              # work entries, then the scan
    work, scan = table[:2 * n_work], table[2 * n_work:]
    ws = torch.empty(lib.grafp_identify_tempo_items_workspace(n_work, top), dtype=torch.uint8, device=dev)
    with _timed(name, (n_items, max_len, k, n_work)):
        check(lib.grafp_identify_tempo_items_f32(_p(index_rows), index_rows.shape[0], _p(first), first.numel() - 1,
                                                 _p(q_rows), q_rows.shape[0], _p(topk_ids), k, _p(item_row),
                                                 _p(item_len), n_items, max_len, top, min_overlap,
                                                 ctypes.cast(nums, ctypes.c_void_p), len(ratios), _p(work), n_work,
                                                 _p(scan), max_cnt, _p(ws), *(_p(o) for o in outs), _stream()), name)
    return outs


IDENTIFY_PQ_M = (16, 32, 64, 128)                                      # identify_pq.hip's sub-quantiser counts


def _pq_args(name, list_id, codes, centroids, codebooks):
    """The shape and dtype checks of a library held as IVF-PQ codes (ops.identify_pq, ops.cross_match_pq)
    -> (n rows, M sub-quantisers, nlist)."""
    if codes.dim() != 2 or codes.dtype != torch.uint8:
        raise ValueError(f"{name}: codes must be (n, M) uint8, not {tuple(codes.shape)} {codes.dtype}")
    n, M = int(codes.shape[0]), int(codes.shape[1])
    if M not in IDENTIFY_PQ_M:
        raise ValueError(f"{name}: M={M} sub-quantisers, not one of {IDENTIFY_PQ_M}")
    if list_id.dtype != torch.int32 or tuple(list_id.shape) != (n,):
        raise ValueError(f"{name}: list_id must be ({n},) int32, not {tuple(list_id.shape)} {list_id.dtype}")
    if centroids.dim() != 2 or centroids.shape[0] < 1 or centroids.shape[1] != 128:
        raise ValueError(f"{name}: centroids must be (nlist, 128), not {tuple(centroids.shape)}")
    if tuple(codebooks.shape) != (M, 256, 128 // M):
        raise ValueError(f"{name}: codebooks must be {(M, 256, 128 // M)} for M={M}, not {tuple(codebooks.shape)}")
    return n, M, int(centroids.shape[0])


def _check_list_ids(name, list_id, nlist):
    """Refuses list ids outside [0, nlist) (two host synchronisations)."""
    if not 0 <= int(list_id.min().item()) <= int(list_id.max().item()) < nlist:
        raise ValueError(f"{name}: a list id lies outside [0, {nlist})")


def identify_pq(list_id, codes, centroids, codebooks, track_first_row, q_rows, topk_ids, item_row, item_len, top=5,
                min_overlap=None, max_len=None):
    """ops.identify against a library held as IVF-PQ codes (grafp_identify_pq_f32): library row r is
    centroids[list_id[r]] + the codewords codes[r] names (one f32 add per element), and every output is bit for bit
    what ops.identify returns on those decoded rows.
    list_id (n) int32 in [0, nlist), codes (n, M) uint8 in library row order, centroids (nlist, 128) f32, codebooks
    (M, 256, 128 // M) f32, M one of 16, 32, 64, 128; the other arguments, the results and the meaning of max_len as
    for ops.identify (without max_len the list ids are range-checked on the host too)."""
    # argument checks first (host values only): they hold on any device
    n, M, nlist = _pq_args("identify_pq", list_id, codes, centroids, codebooks)
    on_host = max_len is None                                            # the ranges are checked here, not vouched for
    n_items, k, top, max_len, min_overlap = _identify_args("identify_pq", n, track_first_row, q_rows, topk_ids,
                                                           item_row, item_len, top, min_overlap, max_len)
    if on_host and n_items and n:
        _check_list_ids("identify_pq", list_id, nlist)
    _require_gpu(list_id, codes, centroids, codebooks, q_rows, topk_ids, item_row, item_len)
    list_id, codes = list_id.detach().contiguous(), codes.detach().contiguous()
    centroids, codebooks, q_rows = _f32c(centroids), _f32c(codebooks), _f32c(q_rows)
    first, topk_ids, item_row, item_len, outs = _identify_tensors(codes.device, track_first_row, topk_ids, item_row,
                                                                  item_len, top)
    if n_items == 0:
        return outs
    with _timed("identify_pq", (n_items, max_len, k, M)):
        check(lib.grafp_identify_pq_f32(_p(list_id), _p(codes), n, _p(centroids), nlist, _p(codebooks), M, _p(first),
                                        first.numel() - 1, _p(q_rows), q_rows.shape[0], _p(topk_ids), k, _p(item_row),
                                        _p(item_len), n_items, max_len, top, min_overlap, *(_p(o) for o in outs),
                                        _stream()), "identify_pq")
    return outs


SELF_MATCH_MAX_K, SELF_MATCH_MAX_TOP = 32, 64                            # selfmatch.hip's limits


def _check_match_limits(name, top, k, min_votes, min_overlap):
    """The limits ops.self_match and the cross-match ops share."""
    if not 1 <= top <= SELF_MATCH_MAX_TOP:
        raise ValueError(f"{name}: top={top} not in [1, {SELF_MATCH_MAX_TOP}]")
    if not 1 <= k <= SELF_MATCH_MAX_K:
        raise ValueError(f"{name}: k={k} hits per row exceeds {SELF_MATCH_MAX_K}")
    if int(min_votes) < 1 or int(min_overlap) < 1:
        raise ValueError(f"{name}: min_votes and min_overlap must be at least 1")


def self_match_workspace_bytes(src_rows, k, min_votes):
    """Exact workspace of one ops.self_match launch (grafp_self_match_workspace): src_rows the rows of each source track
    (host), k hits per row."""
    r = np.ascontiguousarray(np.asarray(src_rows, np.int64).reshape(-1))
    return int(lib.grafp_self_match_workspace(_vp(r.ctypes.data) if r.size else None, int(r.size), int(k),
                                              int(min_votes)))


def _self_match_args(name, index_rows, track_first_row, topk_ids, tracks, top, min_votes, min_overlap):
    """The host checks ops.self_match and ops.self_match_tempo share -> (n, track table, source tracks, rows per
    source), the last three host int64 tensors."""
    k = int(topk_ids.shape[1])
    _check_match_limits(name, top, k, min_votes, min_overlap)
    n = int(index_rows.shape[0])
    if n < 1 or int(topk_ids.shape[0]) != n:
        raise ValueError(f"{name}: topk_ids has {int(topk_ids.shape[0])} rows for a library of {n}")
    first_h = check_track_table(track_first_row, n)
    T = first_h.numel() - 1
    src = torch.arange(T, dtype=torch.int64) if tracks is None else \
        torch.as_tensor(tracks).detach().to("cpu", torch.int64).reshape(-1)
    if src.numel() and (int(src.min()) < 0 or int(src.max()) >= T):
        raise ValueError(f"{name}: source tracks must lie in [0, {T})")
    lens = (first_h[1:] - first_h[:-1])[src]
    if lens.numel() and int(lens.max()) * k > 2 ** 31 - 1:
        raise ValueError(f"{name}: a track of {int(lens.max())} rows has more than 2^31 - 1 hits at k={k} "
                         "(votes are int32)")
    return n, first_h, src, lens


def self_match(index_rows, track_first_row, topk_ids, tracks=None, top=8, min_votes=4, min_overlap=1):
    """Shared audio inside a track-indexed library (grafp_self_match_f32, one workgroup per source track): for every
    source track a, the `top` other tracks b its rows reappear in, each at its best alignment.
    index_rows (n,128) f32 resident library, track_first_row (T+1) int64 (track t = rows [first[t], first[t+1])),
    topk_ids (n,k) int64 every library row's hits from searching the library against itself (-1: no hit), tracks the
    source tracks (default all).  A hit of row first[a] + i on row first[b] + j (b != a) votes for (b, delta = j - i);
    a candidate's span runs from its first to its last voting i (m rows) and it needs min_votes votes and m >=
    min_overlap rows.  It scores the mean dot product over its whole span (the arithmetic order of ops.identify).
    Returns (track, delta, start, length, score, votes), each (n_src, top) -- int32 but score f32 --, best first,
    padded with -1 / INT_MIN / -1 / 0 / -inf / 0.  The table, the sources and the limits are checked on the host."""
    k, top = int(topk_ids.shape[1]), int(top)
    n, first_h, src, lens = _self_match_args("self_match", index_rows, track_first_row, topk_ids, tracks, top, min_votes,
                                             min_overlap)
    T = first_h.numel() - 1
    _require_gpu(index_rows, topk_ids)
    index_rows = _f32c(index_rows)
    dev = index_rows.device
    first = first_h.to(dev)
    topk_ids = topk_ids.to(torch.int64).contiguous()
    n_src = src.numel()
    src_d = src.to(device=dev, dtype=torch.int32)
    outs = tuple(torch.empty((n_src, top), dtype=torch.float32 if j == 4 else torch.int32, device=dev)
                 for j in range(6))
    if n_src == 0:
        return outs
    ws = torch.empty(self_match_workspace_bytes(lens.numpy(), k, min_votes), dtype=torch.uint8, device=dev)
    with _timed("self_match", (n_src, int(lens.sum()), k)):
        check(lib.grafp_self_match_f32(_p(index_rows), n, _p(first), T, _p(topk_ids), k, _p(src_d), n_src, top, int(min_votes), int(min_overlap), _p(ws), ws.numel(),
                                       *(_p(o) for o in outs), _stream()), "self_match")
    return outs


def _cross_match_args(name, n, track_first_row, q_rows, src_first_row, topk_ids, top, min_votes, min_overlap):
    """The host checks ops.cross_match and ops.cross_match_pq share -> (track table, source table, rows per source),
    host int64 tensors."""
    k = int(topk_ids.shape[1])
    _check_match_limits(name, top, k, min_votes, min_overlap)
    if n < 1:
        raise ValueError(f"{name}: a library of {n} rows")
    if q_rows.dim() != 2 or q_rows.shape[1] != 128:
        raise ValueError(f"{name}: q_rows must be (n_q, 128), not {tuple(q_rows.shape)}")
    n_q = int(q_rows.shape[0])
    if topk_ids.dim() != 2 or int(topk_ids.shape[0]) != n_q:
        raise ValueError(f"{name}: topk_ids has {int(topk_ids.shape[0])} rows for {n_q} source rows")
    first_h = check_track_table(track_first_row, n)
    src_h = torch.as_tensor(src_first_row).detach().to("cpu", torch.int64).reshape(-1)
    if src_h.numel() < 1 or int(src_h[0]) != 0 or int(src_h[-1]) != n_q or bool((src_h[1:] < src_h[:-1]).any()):
        raise ValueError(f"{name}: the source table must run from 0 to n_q = {n_q} and never decrease")
    lens = src_h[1:] - src_h[:-1]
    if lens.numel() and int(lens.max()) * k > 2 ** 31 - 1:
        raise ValueError(f"{name}: a source of {int(lens.max())} rows has more than 2^31 - 1 hits at k={k} "
                         "(votes are int32)")
    if n + (int(lens.max()) if lens.numel() else 0) >= 2 ** 32 or max(n, n_q) >= 0x7fffff00:
        raise ValueError(f"{name}: n={n} library rows and n_q={n_q} source rows exceed the 32-bit alignment of a hit key")
    return first_h, src_h, lens


def _cross_match_outs(n_src, top, dev):
    """The six (n_src, top) results, holding the padding (what sources without rows get)."""
    pad = (-1, -2 ** 31, -1, 0, float("-inf"), 0)
    return tuple(torch.full((n_src, top), pad[j], dtype=torch.float32 if j == 4 else torch.int32, device=dev)
                 for j in range(6))


def cross_match(index_rows, track_first_row, q_rows, src_first_row, topk_ids, top=8, min_votes=4, min_overlap=1):
    """What recordings held outside a track-indexed library share with it (grafp_cross_match_f32, one workgroup per
    source): ops.self_match with the sources taken from q_rows instead of the library.
    index_rows (n,128) f32 resident library, track_first_row (T+1) int64, q_rows (n_q,128) f32 the rows of S sources
    laid end to end, src_first_row (S+1) int64 (source s = rows [src_first[s], src_first[s+1]); first 0, last n_q),
    topk_ids (n_q,k) int64 every source row's hits from searching the library (-1 or outside [0, n): no hit).
    Row i of a source with hit first[b] + j votes for (b, delta = j - i); nothing is dropped.  Spans, eligibility, the
    score, the per-partner best and the order are ops.self_match's, and so are the six (S, top) results and their
    padding.  The tables and the limits are checked on the host."""
    top, k = int(top), int(topk_ids.shape[1])
    n = int(index_rows.shape[0])
    first_h, src_h, lens = _cross_match_args("cross_match", n, track_first_row, q_rows, src_first_row, topk_ids, top,
                                             min_votes, min_overlap)
    _require_gpu(index_rows, q_rows, topk_ids)
    index_rows, q_rows = _f32c(index_rows), _f32c(q_rows)
    dev = index_rows.device
    n_src = lens.numel()
    outs = _cross_match_outs(n_src, top, dev)
    if n_src == 0 or q_rows.shape[0] == 0:
        return outs
    first, src = first_h.to(dev), src_h.to(dev)
    topk_ids = topk_ids.to(torch.int64).contiguous()
    ws = torch.empty(self_match_workspace_bytes(lens.numpy(), k, min_votes), dtype=torch.uint8, device=dev)
    with _timed("cross_match", (n_src, int(lens.sum()), k)):
        check(lib.grafp_cross_match_f32(_p(index_rows), n, _p(first), first.numel() - 1, _p(q_rows), q_rows.shape[0],
                                        _p(src), n_src, _p(topk_ids), k, top, int(min_votes), int(min_overlap), _p(ws),
                                        ws.numel(), *(_p(o) for o in outs), _stream()), "cross_match")
    return outs


def cross_match_half(index_rows_bf16, track_first_row, q_rows, src_first_row, topk_ids, top=8, min_votes=4,
                     min_overlap=1):
    """ops.cross_match against a library held as bf16 rows (grafp_cross_match_half_f32): index_rows_bf16 (n, 128)
    contiguous torch.bfloat16, and every output is bit for bit what ops.cross_match returns on index_rows_bf16.float().
    The other arguments and the results as for ops.cross_match."""
    index_rows_bf16 = _half_rows("cross_match_half", index_rows_bf16)
    top, k = int(top), int(topk_ids.shape[1])
    n = int(index_rows_bf16.shape[0])
    first_h, src_h, lens = _cross_match_args("cross_match_half", n, track_first_row, q_rows, src_first_row, topk_ids,
                                             top, min_votes, min_overlap)
    _require_gpu(index_rows_bf16, q_rows, topk_ids)
    q_rows = _f32c(q_rows)
    dev = index_rows_bf16.device
    n_src = lens.numel()
    outs = _cross_match_outs(n_src, top, dev)
    if n_src == 0 or q_rows.shape[0] == 0:
        return outs
    first, src = first_h.to(dev), src_h.to(dev)
    topk_ids = topk_ids.to(torch.int64).contiguous()
    ws = torch.empty(self_match_workspace_bytes(lens.numpy(), k, min_votes), dtype=torch.uint8, device=dev)
    with _timed("cross_match_half", (n_src, int(lens.sum()), k)):
        check(lib.grafp_cross_match_half_f32(_p(index_rows_bf16), n, _p(first), first.numel() - 1, _p(q_rows),
                                             q_rows.shape[0], _p(src), n_src, _p(topk_ids), k, top, int(min_votes),
                                             int(min_overlap), _p(ws), ws.numel(), *(_p(o) for o in outs), _stream()),
              "cross_match_half")
    return outs


CROSS_MATCH_TEMPO_MAX_ROWS = 4194303                                    # rows per source: i * 512 + 128 fits an int32


def _tempo_ratio_list(name, ratio_num):
    """The ratio checks ops.identify_tempo and the two tempo match ops share -> the ratios as a list of ints."""
    ratios = [int(v) for v in torch.as_tensor(ratio_num).reshape(-1).tolist()]
    if not 1 <= len(ratios) <= IDENTIFY_TEMPO_MAX_RATIOS:
        raise ValueError(f"{name}: {len(ratios)} ratios, not 1 to {IDENTIFY_TEMPO_MAX_RATIOS}")
    if any(b <= a for a, b in zip(ratios, ratios[1:])):
        raise ValueError(f"{name}: ratio_num must be strictly ascending")
    if not all(IDENTIFY_TEMPO_MIN <= v <= IDENTIFY_TEMPO_MAX for v in ratios):
        raise ValueError(f"{name}: every ratio must lie in [{IDENTIFY_TEMPO_MIN}, {IDENTIFY_TEMPO_MAX}] "
                         f"(got {min(ratios)} .. {max(ratios)})")
    return ratios


def _tempo_match_limits(name, ratio_num, top, n, lens):
    """The limits ops.cross_match_tempo and ops.self_match_tempo add to their dense forms' (lens: the rows of each
    source, a host tensor) -> the ratios as a list of ints."""
    ratios = _tempo_ratio_list(name, ratio_num)
    if len(ratios) * top > 4096:
        raise ValueError(f"{name}: {len(ratios)} ratios x top={top} exceed the 4096 slots of the merge")
    longest = int(lens.max()) if lens.numel() else 0
    if longest > CROSS_MATCH_TEMPO_MAX_ROWS:
        raise ValueError(f"{name}: a source of {longest} rows exceeds {CROSS_MATCH_TEMPO_MAX_ROWS}")
    if n + 2 * longest >= 1 << 32:
        raise ValueError(f"{name}: n={n} library rows and a source of {longest} reach past the 2^32 "
                         "alignments a key holds")
    return ratios


def cross_match_tempo_workspace_bytes(src_rows, k, min_votes, n_ratios, top):
    """Exact workspace of one ops.cross_match_tempo launch (grafp_cross_match_tempo_workspace): one header, one copy of
    ops.self_match_workspace_bytes' per-source regions per ratio, six (n_ratios, n_src, top) list arrays."""
    r = np.ascontiguousarray(np.asarray(src_rows, np.int64).reshape(-1))
    return int(lib.grafp_cross_match_tempo_workspace(_vp(r.ctypes.data) if r.size else None, int(r.size), int(k),
                                                     int(min_votes), int(n_ratios), int(top)))


def cross_match_tempo(index_rows, track_first_row, q_rows, src_first_row, topk_ids, ratio_num, top=8, min_votes=4,
                      min_overlap=1):
    """ops.cross_match for recordings that play faster or slower than the catalogue (grafp_cross_match_tempo_f32: one
    workgroup per source and ratio, then one per source that merges the ratios' lists).  ratio_num as for
    ops.identify_tempo: 1 to 64 strictly ascending integers in [128, 512] (host values), each num / 256 track seconds
    per recording second.  At ratio num row i of a source (counted from the source's row 0) sits w(i) = (i * num + 128)
    >> 8 library rows after the source's row 0.  A hit r of row i names the track b holding r and the alignment a = r -
    w(i); a candidate is a unique (b, a, num); votes, span [i_lo, i_hi], m and eligibility as for ops.cross_match, and the
    score is the mean of <q[i], row[a + w(i)]> over i = i_lo .. i_hi in ops.identify's arithmetic order.  Per partner the
    best candidate over all ratios: highest score, then the ratio nearer to 1 (smaller |num - 256|, then smaller num),
    then the smaller a.
    Returns (track, delta = a - first[b], start = i_lo, length = m, score, votes, ratio int32 = num), each (S, top),
    padded with -1 / INT_MIN / -1 / 0 / -inf / 0 / 0; at ratio_num = [256] the first six are ops.cross_match's bit for
    bit.  Limits: ops.cross_match's, sources of at most 4 194 303 rows, n + 2 * (longest source) < 2^32."""
    top, k = int(top), int(topk_ids.shape[1])
    n = int(index_rows.shape[0])
    first_h, src_h, lens = _cross_match_args("cross_match_tempo", n, track_first_row, q_rows, src_first_row, topk_ids,
                                             top, min_votes, min_overlap)
    ratios = _tempo_match_limits("cross_match_tempo", ratio_num, top, n, lens)
    _require_gpu(index_rows, q_rows, topk_ids)
    index_rows, q_rows = _f32c(index_rows), _f32c(q_rows)
    dev = index_rows.device
    n_src = lens.numel()
    outs = _cross_match_outs(n_src, top, dev) + (torch.zeros((n_src, top), dtype=torch.int32, device=dev),)
    if n_src == 0 or q_rows.shape[0] == 0:
        return outs
    first, src = first_h.to(dev), src_h.to(dev)
    topk_ids = topk_ids.to(torch.int64).contiguous()
    nums = (ctypes.c_int32 * len(ratios))(*ratios)                       # read by the entry before it returns
    ws = torch.empty(cross_match_tempo_workspace_bytes(lens.numpy(), k, min_votes, len(ratios), top), dtype=torch.uint8,
                     device=dev)
    with _timed("cross_match_tempo", (n_src, int(lens.sum()), k, len(ratios))):
        check(lib.grafp_cross_match_tempo_f32(_p(index_rows), n, _p(first), first.numel() - 1, _p(q_rows),
                                              q_rows.shape[0], _p(src), n_src, _p(topk_ids), k, top, int(min_votes),
                                              int(min_overlap), ctypes.cast(nums, ctypes.c_void_p), len(ratios), _p(ws),
                                              ws.numel(), *(_p(o) for o in outs), _stream()), "cross_match_tempo")
    return outs


def self_match_tempo(index_rows, track_first_row, topk_ids, ratio_num, tracks=None, top=8, min_votes=4, min_overlap=1):
    """ops.self_match for tracks that share audio at another speed (grafp_self_match_tempo_f32: one workgroup per source
    track and ratio, then one per source that merges the ratios' lists).  index_rows, track_first_row, topk_ids and
    tracks as for ops.self_match; ratio_num as for ops.cross_match_tempo: 1 to 64 strictly ascending integers in
    [128, 512] (host values), each num / 256 rows of the partner per row of the source.  At ratio num row i of source
    track a sits w(i) = (i * num + 128) >> 8 rows after the source's row 0.  A hit r of row first[a] + i outside track a
    names the track b holding r and the alignment a_g = r - w(i); a candidate is a unique (b, a_g, num); votes, span
    [i_lo, i_hi], m and eligibility as for ops.self_match, and the score is the mean of <row[first[a] + i],
    row[a_g + w(i)]> over i = i_lo .. i_hi in ops.identify's arithmetic order.  Per partner the best candidate over all
    ratios: highest score, then the ratio nearer to 1 (smaller |num - 256|, then smaller num), then the smaller a_g.
    Returns (track, delta = a_g - first[b], start = i_lo, length = m, score, votes, ratio int32 = num), each
    (n_src, top), padded with -1 / INT_MIN / -1 / 0 / -inf / 0 / 0.  At ratio_num = [256] the first six are
    ops.self_match's bit for bit; for any ratios all seven are ops.cross_match_tempo's on the source tracks' own rows and
    hits with the own-track hits set to -1.  Limits: ops.self_match's and ops.cross_match_tempo's."""
    k, top = int(topk_ids.shape[1]), int(top)
    n, first_h, src, lens = _self_match_args("self_match_tempo", index_rows, track_first_row, topk_ids, tracks, top,
                                             min_votes, min_overlap)
    ratios = _tempo_match_limits("self_match_tempo", ratio_num, top, n, lens)
    _require_gpu(index_rows, topk_ids)
    index_rows = _f32c(index_rows)
    dev = index_rows.device
    n_src = src.numel()
    outs = _cross_match_outs(n_src, top, dev) + (torch.zeros((n_src, top), dtype=torch.int32, device=dev),)
    if n_src == 0:
        return outs
    first = first_h.to(dev)
    topk_ids = topk_ids.to(torch.int64).contiguous()
    src_d = src.to(device=dev, dtype=torch.int32)
    nums = (ctypes.c_int32 * len(ratios))(*ratios)                       # read by the entry before it returns
    ws = torch.empty(cross_match_tempo_workspace_bytes(lens.numpy(), k, min_votes, len(ratios), top), dtype=torch.uint8,
                     device=dev)
    with _timed("self_match_tempo", (n_src, int(lens.sum()), k, len(ratios))):
        check(lib.grafp_self_match_tempo_f32(_p(index_rows), n, _p(first), first.numel() - 1, _p(topk_ids), k, _p(src_d),
                                             n_src, top, int(min_votes), int(min_overlap),
                                             ctypes.cast(nums, ctypes.c_void_p), len(ratios), _p(ws), ws.numel(),
                                             *(_p(o) for o in outs), _stream()), "self_match_tempo")
    return outs


def cross_match_pq(list_id, codes, centroids, codebooks, track_first_row, q_rows, src_first_row, topk_ids, top=8,
                   min_votes=4, min_overlap=1):
    """ops.cross_match against a library held as IVF-PQ codes (grafp_cross_match_pq_f32): library row r is
    centroids[list_id[r]] + the codewords codes[r] names (one f32 add per element), and every output is bit for bit
    what ops.cross_match returns on those decoded rows.  list_id, codes, centroids, codebooks as for ops.identify_pq
    (the list ids are range-checked on the host); the other arguments and the results as for ops.cross_match."""
    top, k = int(top), int(topk_ids.shape[1])
    n, M, nlist = _pq_args("cross_match_pq", list_id, codes, centroids, codebooks)
    first_h, src_h, lens = _cross_match_args("cross_match_pq", n, track_first_row, q_rows, src_first_row, topk_ids,
                                             top, min_votes, min_overlap)
    _check_list_ids("cross_match_pq", list_id, nlist)
    _require_gpu(list_id, codes, centroids, codebooks, q_rows, topk_ids)
    list_id, codes = list_id.detach().contiguous(), codes.detach().contiguous()
    centroids, codebooks, q_rows = _f32c(centroids), _f32c(codebooks), _f32c(q_rows)
    dev = codes.device
    n_src = lens.numel()
    outs = _cross_match_outs(n_src, top, dev)
    if n_src == 0 or q_rows.shape[0] == 0:
        return outs
    first, src = first_h.to(dev), src_h.to(dev)
    topk_ids = topk_ids.to(torch.int64).contiguous()
    ws = torch.empty(self_match_workspace_bytes(lens.numpy(), k, min_votes), dtype=torch.uint8, device=dev)
    with _timed("cross_match_pq", (n_src, int(lens.sum()), k, M)):
        check(lib.grafp_cross_match_pq_f32(_p(list_id), _p(codes), n, _p(centroids), nlist, _p(codebooks), M, _p(first),
                                           first.numel() - 1, _p(q_rows), q_rows.shape[0], _p(src), n_src,
                                           _p(topk_ids), k, top, int(min_votes), int(min_overlap), _p(ws), ws.numel(),
                                           *(_p(o) for o in outs), _stream()), "cross_match_pq")
    return outs


MERGE_LISTS_MAX, MERGE_LISTS_MAX_SLOTS, MERGE_LISTS_MAX_PAYLOAD = 64, 4096, 6      # merge_lists.hip's limits


def merge_track_lists(track, score, payload, track_base, pad, top=None):
    """One list per item from the lists that S shards of a library returned for the same items
    (grafp_merge_track_lists_f32, one workgroup per item; grafp_amd/sharded.py).  Shard s owns the global tracks
    [track_base[s], track_base[s + 1]) and its lists are in the form the identify and match ops write:
    track (S, n_items, L) int32 shard-local track numbers (negative: padding), score (S, n_items, L) f32, payload
    (P, S, n_items, L) int32 the ops' other outputs (identify: offset, votes; identify_tempo: also ratio; cross_match:
    delta, start, length, votes; cross_match_tempo: also ratio; None: P = 0).  track_base: S host ints, non-negative and
    ascending; pad: P host ints, the padding value of each payload.
    The non-padding entries of an item are ranked by score descending, then global track (track_base[s] + track)
    ascending.  Returns (track int32 (n_items, L) global, score f32 (n_items, L), payload int32 (P, n_items, L)), padded
    with -1 / -inf / pad[p]; top (default L, at most L): only the first `top` columns of each.  An item with
    cross_match's -2 mark in any entry gets track -2 in slot 0 and padding elsewhere.
    Limits: 1 <= S <= 64, 1 <= L <= 64, S * L <= 4096, P <= 6.  Nothing is copied to the device and nothing is read
    back: the call is asynchronous and capturable."""
    if track.dim() != 3 or tuple(score.shape) != tuple(track.shape):
        raise ValueError(f"merge_track_lists: track and score must both be (S, n_items, top), not "
                         f"{tuple(track.shape)} and {tuple(score.shape)}")
    S, n_items, L = (int(v) for v in track.shape)
    P = 0 if payload is None else int(payload.shape[0])
    if payload is not None and (payload.dim() != 4 or tuple(payload.shape[1:]) != (S, n_items, L)):
        raise ValueError(f"merge_track_lists: payload must be (P, {S}, {n_items}, {L}), not {tuple(payload.shape)}")
    if not 1 <= S <= MERGE_LISTS_MAX:
        raise ValueError(f"merge_track_lists: S={S} lists per item, not 1 to {MERGE_LISTS_MAX}")
    if not 1 <= L <= 64:
        raise ValueError(f"merge_track_lists: lists of top={L} entries, not 1 to 64")
    if S * L > MERGE_LISTS_MAX_SLOTS:
        raise ValueError(f"merge_track_lists: S={S} lists x top={L} exceed the {MERGE_LISTS_MAX_SLOTS} slots of the merge")
    if P > MERGE_LISTS_MAX_PAYLOAD:
        raise ValueError(f"merge_track_lists: P={P} payloads, not 0 to {MERGE_LISTS_MAX_PAYLOAD}")
    top = L if top is None else int(top)
    if not 1 <= top <= L:
        raise ValueError(f"merge_track_lists: top={top} not in [1, {L}], the length of the lists")
    bases = [int(v) for v in np.asarray(track_base).reshape(-1)]
    pads = [int(v) for v in np.asarray(pad).reshape(-1)]
    if len(bases) != S or len(pads) != P:
        raise ValueError(f"merge_track_lists: {len(bases)} track bases and {len(pads)} pads for S={S} and P={P}")
    if bases[0] < 0 or any(b < a for a, b in zip(bases, bases[1:])) or bases[-1] >= 2 ** 31:
        raise ValueError("merge_track_lists: track_base must be non-negative and ascending")
    if any(not -2 ** 31 <= v < 2 ** 31 for v in pads):
        raise ValueError("merge_track_lists: a pad is no int32")
    _require_gpu(track, score, payload)
    dev = track.device
    track, score = track.to(torch.int32).contiguous(), _f32c(score)
    payload = None if P == 0 else payload.to(torch.int32).contiguous()
    out_t = torch.empty((n_items, L), dtype=torch.int32, device=dev)
    out_s = torch.empty((n_items, L), dtype=torch.float32, device=dev)
    out_p = torch.empty((P, n_items, L), dtype=torch.int32, device=dev)
    if n_items:
        c_bases, c_pads = (ctypes.c_int32 * S)(*bases), (ctypes.c_int32 * max(1, P))(*pads)   # read before the return
        with _timed("merge_track_lists", (S, n_items, L, P)):
            check(lib.grafp_merge_track_lists_f32(_p(track), _p(score), _p(payload), S, n_items, L, P,
                                                  ctypes.cast(c_bases, _vp), ctypes.cast(c_pads, _vp), _p(out_t),
                                                  _p(out_s), _p(out_p) if P else None, _stream()), "merge_track_lists")
    return out_t[:, :top], out_s[:, :top], out_p[:, :, :top]


class _ExactL2Index:
    """What FlatL2Index and HalfL2Index share: the chunks that add() was given, concatenated once at the first use after
    them, the empty index's answer and the numpy-in / numpy-out handling.  A class states _checked(x) (add's input ->
    the device tensor it keeps), _derive(db) -> (squared norms, bf16 copy or None) and _search(db, sq, q, k)."""

    def __init__(self, d, device, id_base):
        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} needs a HIP device: there is no CPU fallback")
        self.d, self.id_base, self.ntotal = d, int(id_base), 0
        self.device = torch.device(device if device is not None else "cuda")
        self._chunks, self._db, self._sq, self._bf16 = [], None, None, None

    def add(self, x):
        t = self._checked(x)
        self._chunks.append(t)
        self.ntotal += t.shape[0]
        self._db = None

    def _materialise(self):
        if self._db is None:
            self._db = self._chunks[0] if len(self._chunks) == 1 else torch.cat(self._chunks, dim=0)
            self._chunks = [self._db]
            self._sq, self._bf16 = self._derive(self._db)
        return self._db, self._sq

    def held_tensors(self):
        """Every device tensor the index holds once it is searchable (its share of FingerprintLibrary.nbytes)."""
        return [t for t in (*self._materialise(), self._bf16) if t is not None] if self.ntotal else []

    def search(self, q, k):
        """numpy in -> numpy out (D float32 (nq,k), I int64 (nq,k)), like faiss; tensors in -> tensors out."""
        as_numpy = isinstance(q, np.ndarray)
        qt = torch.as_tensor(np.ascontiguousarray(q) if as_numpy else q).to(self.device, dtype=torch.float32)
        if self.ntotal == 0:
            D = torch.full((qt.shape[0], k), float("inf"), device=self.device)
            I = torch.full((qt.shape[0], k), -1, dtype=torch.int64, device=self.device)
        else:
            D, I = self._search(*self._materialise(), qt.reshape(-1, self.d), k)
        return (D.cpu().numpy(), I.cpu().numpy()) if as_numpy else (D, I)


class FlatL2Index(_ExactL2Index):
    """Drop-in for the subset of faiss.IndexFlatL2 that eval.py uses: d, ntotal, add(x), search(q, k).
    The database lives in HBM; `add` also computes the per-row squared norms once."""

    def __init__(self, d=128, device=None, id_base=0, prefilter=True):
        super().__init__(d, device, id_base)
        self.prefilter = bool(prefilter)     # bf16 pre-filter scan + exact rescoring (same results, 2-4x faster)
        self.nprobe = 1            # attribute assigned at eval.py:122; meaningless for exact search

    def _checked(self, x):
        t = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
        return t.to(self.device, dtype=torch.float32).reshape(-1, self.d).contiguous()

    def _derive(self, db):
        return row_sqnorm(db), rows_to_bf16(db) if self.prefilter else None

    def rows(self):
        """The resident (ntotal, d) f32 database tensor (what faiss calls reconstruct_n(0, ntotal))."""
        return self._materialise()[0]

    def _search(self, db, sq, q, k):
        return search_l2(db, sq, q, k, self.id_base, db_bf16=self._bf16)


class HalfL2Index(_ExactL2Index):
    """FlatL2Index for a database held as bf16 rows only: d, ntotal, add(rows_bf16), search(q, k); 260 bytes a row with
    the norm, and no rows() in f32.  With U = the rows' f32 values (exact) every search answers bit for bit as a
    FlatL2Index over U does.  The index shares the rows tensor it is given and copies nothing (several add() calls are
    concatenated once, at the first search after them)."""

    def __init__(self, d=128, device=None, id_base=0):
        super().__init__(d, device, id_base)
        if d != 128:
            raise ValueError(f"HalfL2Index: d={d} unsupported (fingerprints are 128-d)")

    def _checked(self, rows_bf16):
        t = _half_rows("HalfL2Index.add", rows_bf16)
        _require_gpu(t)
        return t

    def _derive(self, db):
        return row_sqnorm_half(db), None

    def half_rows(self):
        """The resident (ntotal, 128) bf16 database tensor: the one tensor add() was given, when it was one."""
        return self._materialise()[0]

    @property
    def nbytes(self):
        """Device bytes of the index: 260 a row."""
        return sum(t.numel() * t.element_size() for t in self.held_tensors())

    def _search(self, db, sq, q, k):
        return search_l2_half(db, sq, q, k, self.id_base)
