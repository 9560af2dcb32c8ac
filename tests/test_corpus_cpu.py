"""CPU tests of the device-resident corpus (grafp_amd/data.py, csrc/corpus.hip): the resampling filter, WAV decoding,
source listing, the epoch plan and the shipped assembly of the new kernels.  No GPU call is made."""
import json
import math
import os
import re
import wave

import numpy as np
import pytest
import torch

from _common import shipped_asm
from grafp_amd import data, ops

RATES = (44100, 48000, 22050, 32000, 8000, 11025)


def _taps_f64(orig_fs, new_fs):
    """The issue's formula, restated term by term in f64 with plain Python math."""
    g = math.gcd(orig_fs, new_fs)
    orig, new = orig_fs // g, new_fs // g
    base = min(orig, new) * 0.99
    width = math.ceil(6 * orig / base)
    K = 2 * width + orig
    taps = np.empty((new, K))
    for p in range(new):
        for k in range(K):
            t = (-p / new + (k - width) / orig) * base
            t = min(max(t, -6.0), 6.0)
            w = math.cos(t * math.pi / 12) ** 2
            taps[p, k] = (1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)) * w * base / orig
    return orig, new, width, K, taps


@pytest.mark.parametrize("orig_fs", RATES)
def test_resample_filter_matches_the_f64_formula(orig_fs):
    orig, new, width, K, want = _taps_f64(orig_fs, 16000)
    o, n, w, taps = ops.resample_filter(orig_fs, 16000)
    assert (o, n, w) == (orig, new, width) and taps.shape == (new, K) and taps.dtype == np.float32
    # rounded once from f64: within half an f32 ulp of the f64 value (plus the libm difference of sin/cos)
    err = np.abs(taps.astype(np.float64) - want)
    assert err.max() <= 1e-7 * max(1.0, np.abs(want).max()), err.max()


def test_filter_sizes_and_output_length():
    assert ops.resample_filter(44100, 16000)[:3] == (441, 160, 17)
    assert ops.resample_filter(44100, 16000)[3].shape[1] == 475
    assert ops.resample_filter(48000, 16000)[:3] == (3, 1, 19)
    assert ops.resample_filter(8000, 16000)[:3] == (1, 2, 7)
    for fs in RATES:
        orig, new, _, _, _ = _taps_f64(fs, 16000)
        for L in (0, 1, 2, orig - 1, orig, 3 * orig + 1, 30 * fs):
            assert ops.resampled_length(L, fs, 16000) == -(-new * L // orig)
    assert ops.resampled_length(30 * 44100, 44100, 16000) == 30 * 16000


def _write_wav(path, a, fs, bits):
    """a: (frames, channels) float in [-1, 1) -> integer PCM WAV."""
    if bits == 8:
        raw = np.clip(np.round(a * 128 + 128), 0, 255).astype(np.uint8).tobytes()
    elif bits == 16:
        raw = np.clip(np.round(a * 32768), -32768, 32767).astype("<i2").tobytes()
    elif bits == 24:
        v = np.clip(np.round(a * 8388608), -8388608, 8388607).astype(np.int64).reshape(-1) & 0xFFFFFF
        raw = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], 1).astype(np.uint8).tobytes()
    else:
        raw = np.clip(np.round(a.astype(np.float64) * 2147483648), -2147483648, 2147483647).astype("<i4").tobytes()
    with wave.open(path, "wb") as w:
        w.setnchannels(a.shape[1])
        w.setsampwidth(bits // 8)
        w.setframerate(fs)
        w.writeframes(raw)


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
@pytest.mark.parametrize("channels", [1, 2])
def test_wav_decode_scaling_and_downmix(tmp_path, bits, channels):
    rng = np.random.default_rng(bits + channels)
    levels = 1 << (bits - 1)
    ints = rng.integers(-levels, levels, size=(1000, channels))
    a = ints / levels
    p = str(tmp_path / "x.wav")
    _write_wav(p, a, 44100, bits)
    got, rate = data.read_wav(p)
    assert rate == 44100 and got.shape == (channels, 1000) and got.dtype == np.float32
    # torchaudio.load's scaling: unsigned 8-bit (x - 128) / 128, signed n-bit x / 2^(n-1)
    np.testing.assert_array_equal(got, (ints.T / levels).astype(np.float32))
    mono, rate = data.read_audio(p, 16000)
    want = torch.from_numpy((ints.T / levels).astype(np.float32)).mean(dim=0).numpy()
    np.testing.assert_array_equal(mono, want)
    assert data.wav_info(p) == (44100, 1000)


def test_sources_json_index_order_and_directory(tmp_path):
    for name in ("b.wav", "a.wav", "sub/c.wav"):
        os.makedirs(os.path.dirname(str(tmp_path / name)), exist_ok=True)
        _write_wav(str(tmp_path / name), np.zeros((10, 1)), 16000, 16)
    np.save(str(tmp_path / "d.npy"), np.zeros(5, np.float32))
    listed = data.list_source(str(tmp_path))
    assert [os.path.relpath(p, str(tmp_path)) for p in listed] == ["a.wav", "b.wav", "d.npy", "sub/c.wav"]
    idx = {"2": str(tmp_path / "a.wav"), "0": str(tmp_path / "sub/c.wav"), "1": str(tmp_path / "b.wav"),
           "10": str(tmp_path / "d.npy")}
    ip = str(tmp_path / "index.json")
    json.dump(idx, open(ip, "w"))
    assert data.list_source(ip) == [idx["0"], idx["1"], idx["2"], idx["10"]]
    assert data.list_source([idx["1"], idx["0"]]) == [idx["1"], idx["0"]]


def test_mp3_stem_fallback_and_refusal(tmp_path):
    _write_wav(str(tmp_path / "has_wav.wav"), np.zeros((10, 1)), 16000, 16)
    np.save(str(tmp_path / "has_npy.npy"), np.zeros(5, np.float32))
    paths = [str(tmp_path / "has_wav.mp3"), str(tmp_path / "has_npy.mp3"), str(tmp_path / "none.mp3"),
             str(tmp_path / "plain.wav")]
    with pytest.raises(ValueError, match=r"1 of 4 tracks cannot be decoded.*\.mp3.*2 were replaced"):
        data.resolve_files(paths)
    files, report = data.resolve_files(paths, skip_undecodable=True)
    assert files == [str(tmp_path / "has_wav.wav"), str(tmp_path / "has_npy.npy"), str(tmp_path / "plain.wav")]
    assert report == {"substituted": 2, "skipped": [str(tmp_path / "none.mp3")]}


def test_epoch_plan_disjoint_drop_last_and_shared_across_ranks():
    n, B, W = 103, 8, 3
    plans = [data.epoch_plan(n, B, torch.Generator().manual_seed(5), r, W) for r in range(W)]
    assert all(len(p) == n // (B * W) == 4 for p in plans)
    rows = torch.cat([torch.cat(p) for p in plans])
    assert rows.numel() == 4 * B * W and rows.unique().numel() == rows.numel()          # disjoint, drop-last
    assert rows.min() >= 0 and rows.max() < n
    # the same seed gives every rank the same permutation: the union of the ranks' step s is one contiguous slice
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    for s in range(4):
        got = torch.cat([plans[r][s] for r in range(W)])
        assert torch.equal(got, perm[s * B * W:(s + 1) * B * W])
    again = data.epoch_plan(n, B, torch.Generator().manual_seed(5), 1, W)
    assert all(torch.equal(a, b) for a, b in zip(again, plans[1]))
    with pytest.raises(ValueError):
        data.epoch_plan(n, B, None, 3, 3)


def test_corpus_kernels_have_no_packed_high_register_select():
    """The shipped object's own command (make -n), compiled to device assembly: no packed-f32 instruction at all in
    corpus.hip, so none whose low lane reads the high register of a pair."""
    asm = shipped_asm("corpus")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert any("resample_kernel" in k for k in kernels) and any("draw_pairs_kernel" in k for k in kernels)
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm
