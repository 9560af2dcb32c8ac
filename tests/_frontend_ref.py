"""float64 restatements of the audio front end (log-mel, whole-track segmentation, peak extractor): the contract the
kernels of logmel.hip and peak_extract.hip are tested against, plus the cases and inputs that the CPU tests
(test_frontend_cpu.py) and the GPU tests (test_gpu_kernels.py) share.  torch on the CPU, in double; nothing here is
imported from grafp_amd."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from _hashfill import hash_normalish, hash_uniform

FS = 16000
POWER_FLOOR = 1e-10            # AmplitudeToDB's clamp: 10 log10(1e-10) = -100 dB
DB_BAR = 2e-3                  # the project's log-mel bar, dB
POWER_BAR = 4.7e-4             # the same bar as a power ratio: 10^(2e-3 / 10) - 1 = 4.606e-4
LOUD = 1e-4                    # an entry within 40 dB of its frame's loudest band
# The floor term c of the all-entries bound |Pg - Pc| <= POWER_BAR * Pc + c * M.  c_ref is max |P32 - Pc| / M of the f32
# torch path (oracle.model.logmel: pocketfft in f32) against logmel_power64, over every entry of every case below but the
# two "quiet" inputs (at -95 dB one ulp of the f32 dB value is 1.8e-6 in power: there the relative term carries the f32
# path, which is checked too).  Measured on an x86-64 host by test_frontend_cpu.py, which prints it per case: 8.3e-7 at
# most (the 16-band case), rounded up here.  The kernels get 16 x that: four bits for the 31-step twiddle recurrence of the
# register FFT and the radix-2 ordering against pocketfft's mixed radix.
C_REF = 8.5e-7
C_FLOOR = 16 * C_REF           # 1.36e-5


# ---------------------------------------------------------------------------------------------- log-mel
def logmel_power64(x, fs, n_fft, win_len, hop, n_mels):
    """(B, T) waveform -> un-clamped mel power (B, n_mels, 1 + T // hop) in double.  The f32 filterbank table is an input
    of the kernel, not its work: it is widened, not recomputed."""
    from oracle.model import mel_filterbank
    x = torch.as_tensor(x).reshape(-1, np.shape(x)[-1]).to(torch.float64)
    win = torch.hann_window(win_len, periodic=True, dtype=torch.float64)
    spec = torch.stft(x, n_fft, hop_length=hop, win_length=win_len, window=win, center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2                                   # (B, bins, frames)
    fb = mel_filterbank(n_fft // 2 + 1, n_mels, fs).to(torch.float64)         # (bins, n_mels)
    return torch.einsum("bkf,km->bmf", power, fb)


def logmel_errors(db, p64):
    """What the two assertions of the log-mel tests look at, from a dB output and the float64 mel power:
    loud (mask: within 40 dB of the frame's loudest band), db_err (|dB - 10 log10 Pc|), floor_raw (|Pg - Pc| / M) and
    floor_excess ((|Pg - Pc| - POWER_BAR * Pc) / M: the c the all-entries bound would need)."""
    pc = torch.clamp(p64, min=POWER_FLOOR)
    m = pc.amax(dim=1, keepdim=True)
    db = torch.as_tensor(db).to(torch.float64).reshape(pc.shape)
    err = (10.0 ** (db / 10.0) - pc).abs()
    return {"loud": pc >= LOUD * m, "db_err": (db - 10.0 * torch.log10(pc)).abs(),
            "floor_excess": (err - POWER_BAR * pc) / m, "floor_raw": err / m}


# id, (n_fft, win_len, hop, n_mels), B, T, signal
_K1024 = (1024, 1024, 512, 64)
_G512 = (512, 512, 256, 64)
LOGMEL_CASES = (
    # the register-FFT kernel (n_fft 1024, at most 64 bands)
    [(f"r1024-T{T}", _K1024, 2, T, "noise") for T in (513, 1023, 1024, 1535, 16000, 16123)] + [
        ("r1024-40bands", (1024, 1024, 512, 40), 2, 4000, "noise"),
        ("r1024-16bands", (1024, 1024, 512, 16), 2, 4000, "noise"),
        ("r1024-33bands", (1024, 1024, 512, 33), 2, 4000, "noise"),
        ("r1024-win400-hop160", (1024, 400, 160, 64), 2, 4000, "noise"),
        ("r1024-1d", _K1024, 1, 4000, "noise"),
        # the radix-2 Stockham kernel
        ("g256-40bands", (256, 256, 128, 40), 2, 4000, "noise"),
        ("g512", _G512, 2, 4000, "noise"),
        ("g512-win400-hop160", (512, 400, 160, 64), 2, 4000, "noise"),
        ("g2048-128bands", (2048, 2048, 1024, 128), 2, 4000, "noise"),
        ("g1024-128bands", (1024, 1024, 512, 128), 2, 4000, "noise"),
        ("g256-128bands-empty", (256, 256, 128, 128), 2, 4000, "noise"),
        ("g512-T1100", _G512, 2, 1100, "noise"),
    ] + [(f"{k}-{sig}", cfg, 2, 16000, sig) for k, cfg in (("r1024", _K1024), ("g512", _G512))
         for sig in ("dc", "tone", "impulse", "zeros", "quiet")])
LOGMEL_IDS = [c[0] for c in LOGMEL_CASES]


def min_loud_share(case):
    """The share of entries (of bands that have bins) that must be loud, so that the dB assertion is not vacuous: all of
    them on noise, 5 % on the tone (the reference alone gives 8.3 % and 6.7 %).  One noise case cannot reach 100 %: at 128
    bands of 129 bins, 57 bands have a single bin (and 14 have none).  The power of one bin of white noise is exponentially
    distributed, so of these 3648 entries a share of about 1e-4 M / mean lies more than 40 dB under the frame's loudest
    band: 8 of the 7296 entries of bands with bins here, 6 to 14 with other draws.  99.8 % is asked there; the entries
    left out still fall under the all-entries bound."""
    name, signal = case[0], case[4]
    if signal == "noise":
        return 0.998 if name == "g256-128bands-empty" else 1.0
    return 0.05 if signal == "tone" else 0.0


# The noise of a case is named after its id.  At 1024 / 128 bands (bands of two bins) that draw leaves 1 entry of 2048 at
# 0.8e-4 of its frame's loudest band; the draw named here has every entry above 1.0e-3 of it, ten times the threshold.
_NOISE_NAME = {"g1024-128bands": "g1024-128bands.e"}


def logmel_input(case):
    """The (B, T) f32 waveform of a case (a pure function of its id)."""
    name, _cfg, B, T, signal = case
    noise = hash_normalish(f"frontend:logmel.{_NOISE_NAME.get(name, name)}", (B, T))
    if signal == "noise":
        x = 0.1 * noise
    elif signal == "dc":
        x = 0.1 * noise + 0.5
    elif signal == "tone":
        x = np.broadcast_to(0.5 * np.sin(2.0 * np.pi * 1000.0 * np.arange(T) / FS), (B, T))
    elif signal == "impulse":
        x = np.zeros((B, T))
        x[:, 5000] = 1.0
    elif signal == "zeros":
        x = np.zeros((B, T))
    elif signal == "quiet":
        x = 3e-7 * noise
    else:
        raise ValueError(signal)
    return np.ascontiguousarray(x, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _logmel_case_ref(name):
    case = LOGMEL_CASES[LOGMEL_IDS.index(name)]
    x = logmel_input(case)
    return x, logmel_power64(x, FS, *case[1])


def logmel_case_ref(case):
    """(waveform f32 numpy, P64) of a case, computed once per process."""
    return _logmel_case_ref(case[0])


# ---------------------------------------------------------------------------------------------- segmentation
def unfold64(spec, size, step):
    """(n_mels, n_frames) -> (n_seg, n_mels, size); a track shorter than one segment has none."""
    spec = torch.as_tensor(spec)
    if spec.shape[1] < size:
        return spec.new_empty((0, spec.shape[0], size))
    return spec.t().unfold(0, size, step)


UNFOLD_CASES = [(64, 219, 32, 3), (64, 32, 32, 3), (64, 31, 32, 3), (40, 100, 8, 13), (5, 50, 1, 1), (64, 1700, 32, 3)]


# ---------------------------------------------------------------------------------------------- peak extractor
AMBIGUOUS = 1e-4               # |z| below this: the ReLU may fall either way in f32 (ten times the forward tolerance)


def peak_extract64(spec, w, b, stride_h):
    """oracle.model.peak_extract in double: -> (relu(z), z), both (B, F, Ho * W).  z is the conv output before the ReLU.
    The two ramps are f32 tables handed to the kernel, so they are widened like the filterbank above."""
    spec, w, b = (torch.as_tensor(v).to(torch.float64) for v in (spec, w, b))
    B, H, W = spec.shape
    lo = torch.amin(spec, dim=(1, 2), keepdim=True)
    hi = torch.amax(spec, dim=(1, 2), keepdim=True)
    s = (spec - lo) / (hi - lo)
    t_ramp = torch.linspace(0, 1, steps=W).to(torch.float64).view(1, 1, W).expand(B, H, W)
    f_ramp = torch.linspace(0, 1, steps=H).to(torch.float64).view(1, H, 1).expand(B, H, W)
    inp = torch.stack((t_ramp, f_ramp, s), dim=1)
    z = F.conv2d(inp, w, b, stride=(stride_h, 1), padding=(w.shape[2] // 2, w.shape[3] // 2))
    z = z.reshape(B, w.shape[0], -1)
    return F.relu(z), z


# (B, H, W, F, KH, KW, stride_h)
PEAK_FAST = [(3, 64, 32, 8, 7, 7, 2), (2, 63, 32, 8, 7, 7, 2), (2, 128, 32, 8, 7, 7, 2), (2, 64, 32, 8, 7, 7, 1),
             (2, 40, 32, 8, 7, 7, 3), (1, 7, 32, 8, 7, 7, 2), (2, 1, 32, 8, 7, 7, 1)]
PEAK_GENERIC = [(2, 64, 32, 6, 7, 7, 2), (2, 64, 31, 8, 7, 7, 2), (3, 33, 20, 5, 5, 3, 2), (2, 16, 8, 3, 1, 1, 1),
                (2, 24, 12, 4, 9, 3, 2)]
PEAK_MANY = (600, 64, 32, 8, 7, 7, 2)      # more clips than the 512 workgroups of the backward pass
PEAK_SHAPES = PEAK_FAST + PEAK_GENERIC + [PEAK_MANY]


def peak_grad_bar(shape):
    """Relative to max|gradient|.  2e-5 is the project's absolute term; over 600 clips the f32 accumulation costs more
    (the f32 torch path itself measures 5e-6 there) and the bar is 1e-4."""
    return 1e-4 if shape == PEAK_MANY else 2e-5


def peak_inputs(shape):
    B, H, W, nf, KH, KW, _sh = shape
    tag = "x".join(str(v) for v in shape)
    spec = torch.from_numpy(40.0 * hash_uniform(f"frontend:peak.spec.{tag}", (B, H, W)) - 30.0)
    w = torch.from_numpy(0.1 * hash_normalish(f"frontend:peak.w.{tag}", (nf, 3, KH, KW)))
    b = torch.from_numpy(0.05 * hash_normalish(f"frontend:peak.b.{tag}", (nf,)))
    return spec, w, b


@functools.lru_cache(maxsize=None)
def peak_case(shape):
    """Inputs and float64 results of one shape, computed once per process and never modified:
    spec, w, b (f32), out64, z (double), ambiguous (bool), g (f32 upstream gradient, zero where ambiguous), dw64, db64."""
    spec, w, b = peak_inputs(shape)
    w64 = w.to(torch.float64).requires_grad_(True)
    b64 = b.to(torch.float64).requires_grad_(True)
    out64, z = peak_extract64(spec, w64, b64, shape[6])
    ambiguous = z.detach().abs() < AMBIGUOUS
    tag = "x".join(str(v) for v in shape)
    g = torch.from_numpy(hash_normalish(f"frontend:peak.g.{tag}", tuple(out64.shape)))
    g = torch.where(ambiguous, torch.zeros_like(g), g)
    out64.backward(g.to(torch.float64))
    return {"spec": spec, "w": w, "b": b, "out64": out64.detach(), "z": z.detach(), "ambiguous": ambiguous, "g": g,
            "dw64": w64.grad, "db64": b64.grad}


def rel_max(got, want):
    """max|got - want| / max|want| in double."""
    got, want = torch.as_tensor(got).to(torch.float64), torch.as_tensor(want).to(torch.float64)
    return float((got - want).abs().max() / want.abs().max())


def forward_excess(got, want):
    """max of |got - want| - (1e-5 + 1e-4 |want|): <= 0 inside the peak extractor's forward bar."""
    got, want = torch.as_tensor(got).to(torch.float64), torch.as_tensor(want).to(torch.float64)
    return float(((got - want).abs() - (1e-5 + 1e-4 * want.abs())).max())

