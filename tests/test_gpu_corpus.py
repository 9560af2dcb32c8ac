"""The device-resident corpus on the MI355X: grafp_resample_f32 and grafp_draw_pairs_f32 against their CPU
restatements (tests/_corpus_ref.py), the quantile norms, reproducibility, and DeviceAudioCorpus end to end."""
import math
import os
import wave

import numpy as np
import pytest
import torch

from _corpus_ref import draw_pairs_ref, resample_f64, resample_torch_f32
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
