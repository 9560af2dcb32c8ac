"""The device-resident corpus on the MI355X: grafp_resample_f32 and grafp_draw_pairs_f32 against their CPU
restatements (tests/_corpus_ref.py), the quantile norms, reproducibility, and DeviceAudioCorpus end to end; then the
resampler on every launch plan of the table (asserted through grafp_resample_plan) in a poisoned bank, more tracks than
one launch holds, the multi-rate multi-chunk load path, and every branch and edge of the draw, bit for bit.  The
comparisons print their worst deviation (pytest -s)."""
import collections
import math
import os
import wave

import numpy as np
import pytest
import torch

from _corpus_ref import (RESAMPLE_CASES, RESAMPLE_REFUSED, case_id, case_lengths, draw_pairs_ref, quantile_bracket,
                         resample_f64, resample_plan, resample_torch_f32)
from grafp_amd import data, ops
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
RATES = (44100, 48000, 22050, 32000, 8000, 11025)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _lengths(fs):
    orig, new, width, taps = ops.resample_filter(fs, 16000)
    K = taps.shape[1]
    return [1, K - 1, 7 * orig, 30 * fs]


@pytest.mark.parametrize("fs", RATES)
def test_resample_matches_f64_and_torch_restatements(dev, fs):
    g = torch.Generator().manual_seed(fs)
    xs = [0.3 * torch.randn(L, generator=g) for L in _lengths(fs)]
    flat = torch.cat(xs).to(dev)
    lens = torch.tensor([x.numel() for x in xs])
    starts = torch.cumsum(lens, 0) - lens
    y, ys, yl = ops.resample(flat, starts, lens, fs, 16000)
    y = y.cpu()
    for k, x in enumerate(xs):
        got = y[int(ys[k]):int(ys[k]) + int(yl[k])].double().numpy()
        want = resample_f64(x.numpy(), fs, 16000)
        assert got.shape == want.shape == (ops.resampled_length(x.numel(), fs, 16000),)
        bar = 1e-5 * float(x.abs().max())
        assert np.abs(got - want).max() <= bar, (fs, x.numel(), np.abs(got - want).max())
        want32 = resample_torch_f32(x.numpy(), fs, 16000).double().numpy()
        assert np.abs(got - want32).max() <= bar, (fs, x.numel(), np.abs(got - want32).max())


def test_resample_batch_equals_one_launch_per_track(dev):
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(L, generator=g) for L in (44100 * 2 + 17, 5, 475, 44100 // 3, 100000)]
    lens = torch.tensor([x.numel() for x in xs])
    y, ys, yl = ops.resample(torch.cat(xs).to(dev), torch.cumsum(lens, 0) - lens, lens, 44100, 16000)
    for k, x in enumerate(xs):
        one, _, _ = ops.resample(x.to(dev), torch.zeros(1, dtype=torch.int64), lens[k:k + 1], 44100, 16000)
        assert torch.equal(y[int(ys[k]):int(ys[k]) + int(yl[k])], one)


def test_resample_identity_rate_is_bit_exact(dev):
    x = torch.randn(12345, generator=torch.Generator().manual_seed(4)).to(dev)
    lens = torch.tensor([5000, 7345])
    y, ys, yl = ops.resample(x, torch.tensor([0, 5000]), lens, 16000, 16000)
    assert torch.equal(y, x) and yl.tolist() == [5000, 7345]
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.resample(x.cpu(), torch.tensor([0]), torch.tensor([10]), 44100, 16000)


def _planted_corpus(n, fs, seed):
    """Tracks with planted silence so every branch of the draw is taken: loud tracks, tracks whose first 25000 samples
    are silent (some draws rejected), and two consecutive all-zero tracks (rows that start there advance, or exhaust
    their attempts)."""
    g = torch.Generator().manual_seed(seed)
    tracks = []
    for t in range(n):
        y = 0.2 * torch.randn(45000 + 700 * t, generator=g)
        if t % 3 == 1:
            y[:25000] = 0.0
        if t in (2, 3):
            y.zero_()
        tracks.append(y)
    return tracks


def test_draw_pairs_bit_exact_against_restatement(dev):
    cfg = load_config()
    fs = cfg["fs"]
    clip, om = int(fs * cfg["dur"]), int(fs * cfg["offset"] + int(fs * cfg["dur"]))
    tracks = _planted_corpus(6, fs, 7)
    corpus = data.DeviceAudioCorpus(cfg, [t.numpy() for t in tracks], dev)
    assert corpus.stats["excluded"] == 0 and len(corpus.eligible) == 6
    # norms: eps + torch.quantile(|y|, q), as the reference's qtile_norm on the CPU, to 1 ulp
    want_norm = torch.stack([1e-8 + torch.quantile(t.abs(), cfg["norm"]) for t in tracks])
    got_norm = corpus.norms.cpu()
    assert torch.all((got_norm.view(torch.int32) - want_norm.view(torch.int32)).abs() <= 1)
    B, A = 128, 3
    rows = torch.arange(B) % 6
    u = torch.rand((B, A, 3), generator=torch.Generator().manual_seed(8))
    before = corpus.silent_rows()
    x_i, x_j = ops.draw_pairs(corpus.bank, corpus._el_start, corpus._el_len, corpus._el_norm, rows.to(dev), u.to(dev),
                              clip, om, cfg["silence"], corpus._silent)
    ri, rj, silent = draw_pairs_ref([corpus.track(i).cpu() for i in corpus.eligible], corpus.norms.cpu(), rows, u,
                                    clip, om, cfg["silence"])
    assert torch.equal(x_i.cpu(), ri) and torch.equal(x_j.cpu(), rj)
    assert silent > 0 and corpus.silent_rows() - before == silent
    # the branches were taken: some rows advanced past a rejected first attempt, some accepted at once
    first_ok = draw_pairs_ref([corpus.track(i).cpu() for i in corpus.eligible], corpus.norms.cpu(), rows, u[:, :1],
                              clip, om, cfg["silence"])[2]
    assert 0 < first_ok < B


def test_draw_pairs_seeded_generator_repeats(dev):
    cfg = load_config()
    tracks = _planted_corpus(5, cfg["fs"], 9)
    corpus = data.DeviceAudioCorpus(cfg, [t.numpy() for t in tracks], dev)
    a = corpus.draw_pairs([0, 1, 3, 4], generator=torch.Generator(device=dev).manual_seed(1))
    b = corpus.draw_pairs([0, 1, 3, 4], generator=torch.Generator(device=dev).manual_seed(1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = corpus.draw_pairs([0, 1, 3, 4], generator=torch.Generator().manual_seed(1))
    d = corpus.draw_pairs([0, 1, 3, 4], generator=torch.Generator().manual_seed(1))
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])
    steps = list(corpus.batches(2, generator=torch.Generator().manual_seed(2)))
    assert len(steps) == 2 and steps[0][0].shape == (2, 16000)


# ---- resample on every launch plan of the table ---------------------------------------------------------------------------
GAP = 7


@pytest.mark.parametrize("case", RESAMPLE_CASES, ids=case_id)
def test_resample_every_plan_against_f64_in_a_poisoned_bank(dev, case):
    """The plan the launch takes is the table's; tracks of the lengths around the workgroup tile, back to back in one input
    bank, are written into a NaN-filled bank with 7 samples of gap before, between and after them: every track within
    1e-5 max|x| of float64, every gap sample still NaN, and the packed form (no `out`) gives the same bits."""
    rc, p, msg = resample_plan(ops.lib, case.orig_fs, case.new_fs)
    assert rc == 0 and (p.JT, p.n_pb) == (case.JT, case.n_pb), (p, msg)
    orig, new, width, taps = ops.resample_filter(case.orig_fs, case.new_fs)
    lengths = case_lengths(p, orig, taps.shape[1])
    g = torch.Generator().manual_seed(case.orig_fs + case.new_fs)
    xs = [0.3 * torch.randn(L, generator=g) for L in lengths]
    lens = torch.tensor(lengths)
    out_lens = [ops.resampled_length(L, case.orig_fs, case.new_fs) for L in lengths]
    assert out_lens[0] == 0 and out_lens[4] == 64 * p.JT * new and -(-out_lens[5] // new) == 64 * p.JT + 1
    out_starts, pos = [], GAP
    for m in out_lens:
        out_starts.append(pos)
        pos += m + GAP
    out = torch.full((pos,), float("nan"), device=dev)
    flat = torch.cat(xs).to(dev)
    y, ys, yl = ops.resample(flat, torch.cumsum(lens, 0) - lens, lens, case.orig_fs, case.new_fs, out=out,
                             out_starts=torch.tensor(out_starts))
    assert y.data_ptr() == out.data_ptr() and ys.tolist() == out_starts and yl.tolist() == out_lens
    got = out.cpu()
    written = torch.zeros(pos, dtype=torch.bool)
    worst = 0.0
    for k, x in enumerate(xs):
        s, m = out_starts[k], out_lens[k]
        written[s:s + m] = True
        if m == 0:
            continue
        want = resample_f64(x.numpy(), case.orig_fs, case.new_fs)
        assert want.shape == (m,)
        bar = 1e-5 * float(x.abs().max())
        err = float(np.abs(got[s:s + m].double().numpy() - want).max())           # NaN (an unwritten sample) fails the bar
        worst = max(worst, err / bar)
        assert err <= bar, (case, lengths[k], err, bar)
    print(f"resample {case.orig_fs}->{case.new_fs} JT={p.JT} n_pb={p.n_pb} W={p.W}: worst |dev - f64| = {worst:.3f} of the "
          f"bar 1e-5 max|x| (lengths {lengths})")
    assert int((~written).sum()) == GAP * (len(xs) + 1)
    assert bool(torch.isnan(got[~written]).all()), "a sample outside [out_start, out_start + out_len) was written"
    assert not bool(torch.isnan(got[written]).any())
    packed, ps, pl = ops.resample(flat, torch.cumsum(lens, 0) - lens, lens, case.orig_fs, case.new_fs)
    assert pl.tolist() == out_lens and packed.numel() == sum(out_lens)
    assert torch.equal(packed.cpu(), got[written])


@pytest.mark.parametrize("orig_fs,new_fs,window", RESAMPLE_REFUSED)
def test_resample_refuses_a_ratio_whose_window_exceeds_the_lds(dev, orig_fs, new_fs, window):
    out = torch.full((64,), float("nan"), device=dev)
    x = torch.randn(5000, device=dev)
    with pytest.raises(RuntimeError, match=f"{window}-sample window"):
        ops.resample(x, torch.tensor([0]), torch.tensor([5000]), orig_fs, new_fs, out=out, out_starts=torch.tensor([3]))
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(out).all())                      # nothing was launched


def test_resample_more_tracks_than_one_launch_holds(dev):
    """65 537 tracks (grid.y holds 65 535): the loop over launches gives, bit for bit, what two calls of fewer tracks give,
    and the tracks across the launch boundary are within the bar of float64."""
    n = 65537
    g = torch.Generator().manual_seed(65537)
    lens = torch.randint(1, 4, (n,), generator=g)
    starts = torch.cumsum(lens, 0) - lens
    flat_h = 0.3 * torch.randn(int(lens.sum()), generator=g)
    flat = flat_h.to(dev)
    y, ys, yl = ops.resample(flat, starts, lens, 3, 1)
    assert y.numel() == n and yl.tolist() == [1] * n and ys.tolist() == list(range(n))
    cut = 40000
    a, _, _ = ops.resample(flat, starts[:cut], lens[:cut], 3, 1)
    b, _, _ = ops.resample(flat, starts[cut:], lens[cut:], 3, 1)
    assert torch.equal(y, torch.cat([a, b]))
    got = y.cpu().double().numpy()
    worst = 0.0
    for k in range(n - 200, n):                                # 198 tracks of the first launch, 2 of the second
        x = flat_h[int(starts[k]):int(starts[k]) + int(lens[k])]
        want = resample_f64(x.numpy(), 3, 1)
        bar = 1e-5 * float(x.abs().max())
        err = abs(got[k] - want[0])
        worst = max(worst, err / bar)
        assert want.shape == (1,) and err <= bar, (k, err, bar)
    print(f"resample 3->1, 65537 tracks: worst |dev - f64| over the launch boundary = {worst:.3f} of the bar")


# ---- the load path of DeviceAudioCorpus -------------------------------------------------------------------------------------
def test_corpus_load_path_many_rates_and_chunks(dev):
    """Twelve (array, rate) pairs, four rates interleaved, chunk_bytes so small that every rate takes two launches: each
    track lands at its own place in the bank (a wrong scatter order shows here), the tracks tile the bank, the statistics
    and the norms are right."""
    cfg = load_config()
    rates = (44100, 16000, 8000, 48000)
    per_rate = {44100: (3000, 0, 60001), 16000: (2500, 3000, 40000), 8000: (0, 1, 20000), 48000: (5999, 1, 120000)}
    g = torch.Generator().manual_seed(12)
    source = [(0.3 * torch.randn(per_rate[rates[i % 4]][i // 4], generator=g).numpy(), rates[i % 4]) for i in range(12)]
    chunk_bytes = 4 * 6000                                    # the first two tracks of a rate share a launch, the third not
    assert all(4 * (L[0] + L[1]) <= chunk_bytes < 4 * (L[0] + L[1] + L[2]) for L in per_rate.values())
    corpus = data.DeviceAudioCorpus(cfg, source, dev, chunk_bytes=chunk_bytes)
    out_len = [ops.resampled_length(x.size, r, 16000) for x, r in source]
    assert corpus.track_len.tolist() == out_len
    assert corpus.track_start.tolist() == np.concatenate([[0], np.cumsum(out_len)[:-1]]).tolist()          # tile the bank
    assert corpus.bank.numel() == sum(out_len) and len(corpus) == 12
    om = corpus.offset_mod
    assert om == 16800 and corpus.stats["rates"] == {r: 3 for r in rates} and corpus.stats["tracks"] == 12
    assert corpus.stats["excluded"] == sum(m < om + 1 for m in out_len) == 8
    assert corpus.eligible == [i for i in range(12) if out_len[i] >= om + 1]
    for i, (x, r) in enumerate(source):
        got = corpus.track(i).cpu()
        assert got.numel() == out_len[i]
        if r == 16000:
            assert torch.equal(got, torch.from_numpy(x))
        elif x.size:
            want = resample_f64(x, r, 16000)
            assert np.abs(got.double().numpy() - want).max() <= 1e-5 * np.abs(x).max(), (i, r, x.size)
        if out_len[i]:
            want_norm = 1e-8 + torch.quantile(got.abs(), cfg["norm"])
        else:
            want_norm = torch.ones(())
        assert abs(int(corpus.norms[i].cpu().view(torch.int32)) - int(want_norm.view(torch.int32))) <= 1, i


def test_quantile_past_2p24_on_the_device(dev):
    n, q = (1 << 24) + 3, 0.95
    v = torch.rand(n, generator=torch.Generator().manual_seed(24))
    got = float(data._quantile(v.to(dev), q))
    low, high = quantile_bracket(np.sort(v.numpy().astype(np.float64)), q)
    print(f"device quantile n={n} q={q}: {low:.9f} <= {got:.9f} <= {high:.9f}")
    assert low <= got <= high


# ---- every branch and edge of the draw ------------------------------------------------------------------------------------
U_LAST = float(np.nextafter(np.float32(1), np.float32(0)))          # 0.99999994, the largest f32 below 1
DRAW_SHAPES = [(100, 137), (1024, 1025), (3001, 3500), (16000, 40896), (40895, 40896)]


def _draw_tracks(clip, om, n, seed):
    """n = 5: lengths offset_mod + 1, offset_mod, clip, 1 and a long one, back to back in that order (a read past a short
    track's end lands in the next track, not in zeros); the second is quieter than `silence` and the long one starts with
    two windows of zeros, so attempts are rejected.  n = 1: the long track alone.  |y| < 0.2."""
    g = torch.Generator().manual_seed(seed)
    lengths = [om + 1, om, clip, 1, 3 * om + 777] if n == 5 else [3 * om + 777]
    tracks = [0.4 * torch.rand(L, generator=g) - 0.2 for L in lengths]
    tracks[-1][:2 * om] = 0.0
    if n == 5:
        tracks[1] *= 1e-3
        tracks[0][0], tracks[2][0], tracks[3][0] = 0.15, -0.15, 0.15
    return tracks


def _draw_inputs(n, A, seed):
    """32 rows: every start track, the wrapped row_track values, and hand-set uniforms 0, 0.99999994 and 1.0 in each of the
    three slots (for every attempt of those rows)."""
    B = 32
    rows = torch.arange(B, dtype=torch.int32) % n
    rows[9:13] = torch.tensor([-1, -n - 2, n, 3 * n + 1], dtype=torch.int32)
    rows[13:22] = n - 1                                       # the hand-set rows start on the long track, where u0 is used
    u = torch.rand((B, A, 3), generator=torch.Generator().manual_seed(seed))
    for slot in range(3):
        for k, val in enumerate((0.0, U_LAST, 1.0)):
            u[13 + 3 * slot + k, :, slot] = val
    return rows, u


def _run_draw(dev, tracks, norms, rows, u, clip, om, silence, counter):
    lens = torch.tensor([t.numel() for t in tracks])
    bank = torch.cat(tracks).to(dev)
    x_i, x_j = ops.draw_pairs(bank, torch.cumsum(lens, 0) - lens, lens, norms.to(dev), rows.to(dev), u.to(dev), clip, om,
                              silence, counter)
    ri, rj, silent, taken = draw_pairs_ref(tracks, norms, rows, u, clip, om, silence, branches=True)
    assert torch.equal(x_i.cpu(), ri) and torch.equal(x_j.cpu(), rj)
    return silent, taken


@pytest.mark.parametrize("clip,om", DRAW_SHAPES)
@pytest.mark.parametrize("n", [1, 5])
def test_draw_pairs_every_branch_bit_exact(dev, clip, om, n):
    """Both views bit for bit against the reference for A = 1 and A = 8, at silence 0.01 (a mix of accepted, rejected and
    exhausted rows), 0.25 (above every peak: every row exhausts its attempts) and 0 (nothing is silent); the counter rises
    by the reference's count, and None in its place is accepted.  The branches are read off the reference's return."""
    tracks = _draw_tracks(clip, om, n, clip + n)
    norms = 0.5 + torch.rand(n, generator=torch.Generator().manual_seed(n))
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    total, seen = 0, collections.Counter()
    for A in (1, 8):
        rows, u = _draw_inputs(n, A, clip + A)
        for silence, count in ((0.01, True), (0.01, False), (0.25, True), (0.0, True)):
            silent, taken = _run_draw(dev, tracks, norms, rows, u, clip, om, silence, counter if count else None)
            total += silent if count else 0
            assert int(counter.item()) == total
            seen.update({f"A{A}_{k}" if k in ("exhausted", "rejected", "accepted_first", "accepted_later") else k: v
                         for k, v in taken.items()})
            if silence == 0.25:
                assert silent == 32 and taken["exhausted"] == 32 and taken["rejected"] == 32 * (A - 1)
            if silence == 0.0:
                assert silent == 0 and taken["accepted_first"] == 32
    want = {f"u{s}_{k}" for s in range(3) for k in ("zero", "last_below_one", "clamped")}
    want |= {"row_negative", "row_past_n", "A1_exhausted", "A1_accepted_first", "A8_exhausted", "A8_rejected",
             "A8_accepted_first", "A8_accepted_later"}
    if n == 5:
        want |= {"short_track", "zero_padded"}
    assert want <= set(seen), want - set(seen)
    assert total > 64


def test_draw_pairs_refuses_a_window_beyond_the_lds(dev):
    assert ops.DRAW_PAIRS_MAX_WINDOW == 40896
    bank = torch.zeros(50000, device=dev)
    one = torch.tensor([0]), torch.tensor([50000]), torch.ones(1)
    with pytest.raises(RuntimeError, match="window of 40897 samples exceeds the LDS"):
        ops.draw_pairs(bank, *one, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, 3, device=dev), 16000, 40897, 0.0)


def test_draw_pairs_peak_equal_to_silence_is_not_silent(dev):
    """The comparison is a strict < on the f32 the kernel receives: a crop whose peak is exactly f32(silence) is kept, one a
    single f32 step below is silent.  (silence = 0.01 rounds down to f32, so a comparison in double would call both silent.)"""
    clip, om, silence = 100, 137, 0.01
    s32 = np.float32(silence)
    below = np.nextafter(s32, np.float32(0))
    assert float(s32) < silence and below < s32
    sign = torch.where(torch.rand(500, generator=torch.Generator().manual_seed(5)) < 0.5, -1.0, 1.0)
    tracks = [sign * float(s32), sign * float(below)]
    norms = torch.tensor([0.75, 1.5])
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    u = torch.rand((4, 1, 3), generator=torch.Generator().manual_seed(6))
    silent, taken = _run_draw(dev, tracks, norms, torch.tensor([0, 1, 0, 1], dtype=torch.int32), u, clip, om, silence, counter)
    assert silent == 2 == int(counter.item()) and taken["peak_equals_silence"] == 2 and taken["exhausted"] == 2
    # with a second attempt the rows that start on the quieter track move on to the other one
    u2 = torch.rand((4, 2, 3), generator=torch.Generator().manual_seed(7))
    silent, taken = _run_draw(dev, tracks, norms, torch.tensor([0, 1, 0, 1], dtype=torch.int32), u2, clip, om, silence, counter)
    assert silent == 0 and int(counter.item()) == 2 and taken["rejected"] == 2 and taken["peak_equals_silence"] == 4


def _write_wav16(path, x, fs):
    with wave.open(path, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(fs)
        pcm = np.clip(np.round(np.stack([x, 0.5 * x], 1) * 32768), -32768, 32767).astype("<i2")
        w.writeframes(pcm.tobytes())


def test_corpus_end_to_end_44k_wav(dev, tmp_path):
    from grafp_amd.fpdb import create_dummy_db
    from grafp_amd.eval import load_memmap_data
    from grafp_amd.modules.transformations import GPUTransformNeuralfp
    from grafp_amd.train import Trainer, build_model
    cfg = load_config()
    rng = np.random.default_rng(0)
    for i in range(5):
        t = np.arange(44100 * 3 + 4410 * i) / 44100
        x = 0.3 * np.sin(2 * math.pi * (220 + 50 * i) * t) + 0.05 * rng.standard_normal(t.size)
        _write_wav16(str(tmp_path / f"t{i}.wav"), x, 44100)
    _write_wav16(str(tmp_path / "short.wav"), 0.1 * rng.standard_normal(44100 // 2), 44100)
    corpus = data.DeviceAudioCorpus(cfg, str(tmp_path), dev)
    assert corpus.stats["tracks"] == 6 and corpus.stats["excluded"] == 1 and corpus.stats["rates"] == {44100: 6}
    torch.manual_seed(0)
    model = build_model(cfg, device=dev)
    tr = Trainer(cfg, model, dev)
    losses = [float(tr.step(x_i, x_j)) for x_i, x_j in corpus.batches(2, generator=torch.Generator().manual_seed(0))]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)

    model.eval()
    aug = GPUTransformNeuralfp(cfg, None, None, train=False)
    create_dummy_db(corpus.tracks(), augment=aug, model=model, output_root_dir=str(tmp_path), fname="dev", verbose=False)
    ref = []
    for f in corpus.files:
        if os.path.basename(f) == "short.wav":
            continue
        mono, _ = data.read_audio(f, cfg["fs"])
        ref.append(torch.from_numpy(resample_f64(mono, 44100, 16000).astype(np.float32)).view(1, -1))
    create_dummy_db(ref, augment=aug, model=model, output_root_dir=str(tmp_path), fname="ref", verbose=False)
    a, sa = load_memmap_data(str(tmp_path), "dev", display=False)
    b, sb = load_memmap_data(str(tmp_path), "ref", display=False)
    assert tuple(sa) == tuple(sb) and sa[0] > 0
    assert np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-4


def test_load_bank_resamples_only_when_asked(dev, tmp_path):
    from grafp_amd.modules.transformations import load_bank
    rng = np.random.default_rng(1)
    p48, p16 = str(tmp_path / "ir48.wav"), str(tmp_path / "ir16.wav")
    _write_wav16(p48, 0.2 * rng.standard_normal(4800), 48000)
    _write_wav16(p16, 0.2 * rng.standard_normal(1600), 16000)
    with pytest.raises(ValueError):
        load_bank([p48, p16], 16000)
    bank, starts, lens = load_bank([p48, p16], 16000, resample=True)
    assert lens.tolist() == [1600, 1600]
    mono48, _ = data.read_audio(p48, 16000)
    want = resample_f64(mono48, 48000, 16000)
    assert np.abs(bank[:1600].double().numpy() - want).max() <= 1e-5 * np.abs(mono48).max()
    np.testing.assert_array_equal(bank[1600:].numpy(), data.read_audio(p16, 16000)[0])
