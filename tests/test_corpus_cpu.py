"""CPU tests of the device-resident corpus (grafp_amd/data.py, csrc/corpus.hip): the resampling filter, WAV decoding,
source listing, the epoch plan, the resample launch plan of every case of tests/_corpus_ref.py, the draw reference
against a plainer restatement, the quantile past 2^24 elements and the shipped assembly of the kernels.  No GPU call is
made."""
import collections
import ctypes
import json
import math
import os
import re
import wave

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _corpus_ref import (LDS_FLOATS, PHASES, RESAMPLE_CASES, RESAMPLE_REFUSED, case_id, case_lengths, draw_pairs_ref,
                         quantile_bracket, quantile_f64, resample_plan)
from grafp_amd import data, ops
from grafp_amd._lib import lib

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


@pytest.mark.parametrize("case", RESAMPLE_CASES, ids=case_id)
def test_resample_plan_reports_the_tables_plan(case):
    """grafp_resample_plan is a pure host function; resample_launch reads the same one.  JT and n_pb are the table's (worked
    out by hand there); K4, the window and its bytes follow from them and the filter; and the case reaches what its tags
    say: the shrink loop, a JT strictly between 1 and 16, a window within 512 bytes of the whole LDS, a ragged last phase
    block."""
    orig, new, width, taps = ops.resample_filter(case.orig_fs, case.new_fs)
    K = taps.shape[1]
    rc, p, msg = resample_plan(lib, case.orig_fs, case.new_fs)
    assert rc == 0, msg
    assert (p.JT, p.n_pb) == (case.JT, case.n_pb)
    K4 = -(-K // 4) * 4
    W = (64 * p.JT - 1) * orig + K4
    assert (p.K4, p.W, p.lds_bytes, p.blocks, p.tile_in) == (K4, W, 4 * W, 64 * p.JT, 64 * p.JT * orig)
    assert W <= LDS_FLOATS
    JT0 = -(-16 // p.n_pb)
    assert ("shrink" in case.reaches) == (p.JT < JT0)
    if p.JT < JT0:                                        # the loop stopped at the first JT that fits
        assert (64 * (p.JT + 1) - 1) * orig + K4 > LDS_FLOATS
    assert ("intermediate" in case.reaches) == (1 < p.JT < 16)
    assert ("near_full" in case.reaches) == (4 * (LDS_FLOATS - W) < 512)
    assert "ragged" not in case.reaches or new % PHASES != 0
    assert case_lengths(p, orig, K)[-1] == 2 * p.tile_in + orig + 1


def test_resample_plan_reaches_every_regime_by_name():
    tags = collections.Counter(t for c in RESAMPLE_CASES for t in c.reaches.split())
    assert tags["shrink"] >= 3 and tags["intermediate"] >= 3 and tags["near_full"] == 1
    ragged = sorted(ops.resample_filter(c.orig_fs, c.new_fs)[1] % PHASES for c in RESAMPLE_CASES if "ragged" in c.reaches)
    assert ragged == [1, 3, 5, 6, 8]
    by_rate = {(c.orig_fs, c.new_fs): c for c in RESAMPLE_CASES}
    assert by_rate[(49, 8)].JT == 13 and resample_plan(lib, 49, 8)[1].W == 40847
    assert all((fs, 16000) in by_rate for fs in RATES)


@pytest.mark.parametrize("orig_fs,new_fs,window", RESAMPLE_REFUSED)
def test_resample_plan_refuses_a_window_beyond_the_lds(orig_fs, new_fs, window):
    rc, p, msg = resample_plan(lib, orig_fs, new_fs)
    assert rc == -1 and tuple(p) == (0,) * 7
    assert f"rate ratio {new_fs}/{orig_fs}" in msg and f"{window}-sample window" in msg and str(LDS_FLOATS) in msg


def test_resample_plan_checks_its_arguments():
    info = (ctypes.c_int * 8)()
    assert lib.grafp_resample_plan(3, 1, 19, 41, None) == -1 and b"null pointer" in lib.grafp_last_error()
    assert lib.grafp_resample_plan(3, 1, 19, 40, info) == -1 and b"bad filter" in lib.grafp_last_error()
    assert lib.grafp_resample_plan(0, 1, 19, 38, info) == -1 and b"bad filter" in lib.grafp_last_error()


def _draw_pad_and_slice(tracks, norms, row_track, uniforms, clip, om, silence):
    """The draw stated the plain way: pad every track with offset_mod zeros, then slice."""
    n = len(tracks)
    s32 = np.float32(silence)
    xi, xj, count = [], [], 0
    for b in range(uniforms.shape[0]):
        for a in range(uniforms.shape[1]):
            t = (int(row_track[b]) % n + n + a) % n
            yp = np.concatenate([tracks[t].numpy(), np.zeros(om, np.float32)])
            m = tracks[t].numel() - om
            u = uniforms[b, a].numpy().astype(np.float64)
            r = min(int(np.floor(u[0] * m)), m - 1) if m >= 1 else 0
            ri, rj = (min(int(np.floor(v * (om - clip))), om - clip - 1) for v in u[1:])
            ci, cj = yp[r + ri:r + ri + clip], yp[r + rj:r + rj + clip]
            silent = bool(np.abs(ci).max() < s32 or np.abs(cj).max() < s32)
            if not silent or a == uniforms.shape[1] - 1:
                xi.append(ci / np.float32(norms[t]))
                xj.append(cj / np.float32(norms[t]))
                count += silent
                break
    return torch.from_numpy(np.stack(xi)), torch.from_numpy(np.stack(xj)), count


def test_draw_ref_equals_pad_and_slice_on_short_tracks_and_wrapped_rows():
    clip, om, n = 100, 137, 5
    g = torch.Generator().manual_seed(11)
    tracks = [0.2 * torch.randn(L, generator=g) for L in (om + 1, om, clip, 1, 3 * om + 77)]
    tracks[4][:2 * om] = 0.0
    norms = 0.5 + torch.rand(n, generator=g)
    rows = torch.tensor([0, 1, 2, 3, 4, -1, -n - 2, n, 3 * n + 1, -2 * n, 2, 3])
    for A in (1, 4):
        u = torch.rand((rows.numel(), A, 3), generator=g)
        u[0, :, 0], u[1, :, 1], u[2, :, 2] = 1.0, 1.0, 0.0
        got = draw_pairs_ref(tracks, norms, rows, u, clip, om, 0.01, branches=True)
        want = _draw_pad_and_slice(tracks, norms, rows, u, clip, om, 0.01)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2]
        taken = got[3]
        for name in ("short_track", "zero_padded", "row_negative", "row_past_n", "u0_clamped", "u1_clamped", "u2_zero",
                     "accepted_first") + (("exhausted",) if A == 1 else ("rejected", "accepted_later")):
            assert taken[name] > 0, (A, name, taken)
    # Python's sign rule: -1 is the last track, -n - 2 is track n - 2
    one = draw_pairs_ref(tracks, norms, torch.tensor([-1, -n - 2]), torch.full((2, 1, 3), 0.5), clip, om, 0.0)
    assert torch.equal(one[0][0], (tracks[4] / norms[4])[193:193 + clip])          # r = floor(0.5 * 351), ri = 18
    assert one[0][1].abs().max() == 0 and one[2] == 0          # the 1-sample track read from 18 on: zeros, not silent at 0


def test_quantile_f64_reference_is_numpy_quantile():
    v = np.random.default_rng(0).standard_normal(1001).astype(np.float32)
    for q in (0.0, 0.5, 0.95, 0.999, 1.0):
        assert quantile_f64(v, q) == pytest.approx(np.quantile(v.astype(np.float64), q), rel=1e-15, abs=0)


@pytest.fixture(scope="module", params=[(1 << 24) + 3, (1 << 24) + (1 << 23)], ids=["2p24+3", "2p24+2p23"])
def big_sorted(request):
    """(values f32, their sorted f64 copies), shared by the q cases and left unchanged."""
    v = torch.rand(request.param, generator=torch.Generator().manual_seed(request.param))
    return v, np.sort(v.numpy().astype(np.float64))


@pytest.mark.parametrize("q", [0.95, 0.999])
def test_quantile_past_2p24_lies_in_the_derived_bracket(big_sorted, q):
    """data._quantile's second branch (torch.quantile refuses more than 2^24 elements): between the order statistics at
    floor(r) - 3 and floor(r) + 4 of the f64 rank (_corpus_ref.quantile_bracket says why)."""
    v, s = big_sorted
    with pytest.raises(RuntimeError):
        torch.quantile(v, q)
    got = float(data._quantile(v, q))
    low, high = quantile_bracket(s, q)
    print(f"n={v.numel()} q={q}: {low:.9f} <= {got:.9f} <= {high:.9f}; f64 quantile {quantile_f64(s, q):.9f}")
    assert low <= got <= high


def test_quantile_up_to_2p24_is_torch_quantile():
    v = torch.rand(4099, generator=torch.Generator().manual_seed(1))
    for q in (0.95, 0.999):
        got, want = data._quantile(v, q), torch.quantile(v, q)
        assert abs(int(got.view(torch.int32)) - int(want.view(torch.int32))) <= 1


def test_corpus_kernels_have_no_packed_high_register_select():
    """The shipped object's own command (make -n), compiled to device assembly: no packed-f32 instruction at all in
    corpus.hip, so none whose low lane reads the high register of a pair."""
    asm = shipped_asm("corpus")
    kernels = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert any("resample_kernel" in k for k in kernels) and any("draw_pairs_kernel" in k for k in kernels)
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm
