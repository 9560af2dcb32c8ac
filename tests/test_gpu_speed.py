"""Speed augmentation on the MI355X: grafp_speed_change_f32 against the float64 rule and the float32 restatement of its own
route (tests/_speed_ref.py), the transform's cfg keys, the corpus draw at draw_len, and the trainer in eager and graph form.

Error bar of every numeric comparison: e32 = the largest |speed_f32 - speed_f64| over the test's own inputs, computed on
the CPU; the kernel must stay within 8 * e32 of speed_f64 (a few 1e-7 on uniform [-1, 1] input; the factor covers the
device's sinf / cosf being a couple of ulp where numpy's are under one).  A position held in f32, a tap range off by one or
a wrong cut-off is 1e-3 or more."""
import numpy as np
import pytest
import torch

from _corpus_ref import draw_pairs_ref
from _speed_ref import SMALL_RATIOS, batch_refs, clamp_ratio, uniform_rows
from _warp_views import _cfg, _noise_bank, _tracks, _views
from grafp_amd import data, ops
from grafp_amd.modules.transformations import GPUTransformNeuralfp
from grafp_amd.train import Trainer, build_model, synthetic_batch

pytestmark = pytest.mark.gpu
T_OUT = 700                           # not a multiple of the kernel's 1024-output tile, nor of its 256 threads


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _check(name, got, r64, r32):
    e32 = float(np.abs(r32.astype(np.float64) - r64).max())
    err = float(np.abs(got.double().cpu().numpy() - r64).max())
    print(f"{name}: e32 = {e32:.3e}, kernel error = {err:.3e} ({err / e32:.2f} e32)")
    assert e32 > 0 and err <= 8 * e32, (name, err, e32)


@pytest.fixture(scope="module")
def small():
    """Case 1: six clips at the six ratios; (inside) x_offset = pad with no tap in the padding, (edges) x_offset = 0 on
    500 samples: both ends read the zero padding and the last outputs are padding alone."""
    pad, T_in = ops.speed_pad(2.0), ops.speed_input_len(T_OUT, 2.0)
    x = uniform_rows(6, T_in, 21)
    return {"inside": (x, pad, batch_refs(x, SMALL_RATIOS, T_OUT, pad)),
            "edges": (x[:, :500].copy(), 0, batch_refs(x[:, :500], SMALL_RATIOS, T_OUT, 0))}


@pytest.mark.parametrize("which", ("inside", "edges"))
def test_small_shapes_against_the_rule(dev, small, which):
    x, off, (r64, r32) = small[which]
    got = ops.speed_change(torch.from_numpy(x).to(dev), torch.from_numpy(SMALL_RATIOS).to(dev), T_OUT, x_offset=off)
    assert got.shape == (6, T_OUT) and got.dtype == torch.float32
    _check(which, got, r64, r32)
    if which == "edges":
        assert r64[5, 260:].max() == 0 and torch.count_nonzero(got[5, 260:]) == 0     # rho = 2: past the input
        assert torch.count_nonzero(got[5, :240]) > 200
    # a single clip, 1-D in and out
    one = ops.speed_change(torch.from_numpy(x[4]).to(dev), torch.from_numpy(SMALL_RATIOS[4:5]).to(dev), T_OUT, x_offset=off)
    assert one.shape == (T_OUT,) and torch.equal(one, got[4])


def test_strided_rows_in_and_out(dev, small):
    x, off, (r64, r32) = small["inside"]
    T_in = x.shape[1]
    wide = torch.full((6, T_in + 37), float("nan"), device=dev)
    wide[:, 5:5 + T_in] = torch.from_numpy(x).to(dev)
    out = torch.full((6, T_OUT + 11), -7.0, device=dev)
    ratio = torch.from_numpy(SMALL_RATIOS).to(dev)
    ret = ops.speed_change(wide[:, 5:5 + T_in], ratio, T_OUT, x_offset=off, out=out[:, 3:3 + T_OUT])
    assert ret.data_ptr() == out[:, 3:].data_ptr()
    assert torch.equal(ret, ops.speed_change(torch.from_numpy(x).to(dev), ratio, T_OUT, x_offset=off))
    assert bool((out[:, :3] == -7.0).all()) and bool((out[:, 3 + T_OUT:] == -7.0).all())      # nothing outside the rows
    _check("strided", ret, r64, r32)


def test_ratios_are_clamped_and_nan_is_one(dev, small):
    x, off, _ = small["inside"]
    xd = torch.from_numpy(x[:3]).to(dev)
    odd = ops.speed_change(xd, torch.tensor([0.3, 3.0, float("nan")], device=dev), T_OUT, x_offset=off)
    plain = ops.speed_change(xd, torch.tensor([0.5, 2.0, 1.0], device=dev), T_OUT, x_offset=off)
    assert torch.equal(odd, plain)
    more = ops.speed_change(xd, torch.tensor([float("-inf"), float("inf"), -1.0], device=dev), T_OUT, x_offset=off)
    assert torch.equal(more[:2], plain[:2]) and torch.equal(more[2], ops.speed_change(xd[2], torch.tensor([0.5], device=dev),
                                                                                      T_OUT, x_offset=off))
    assert [float(clamp_ratio(r)) for r in (0.3, 3.0, float("nan"))] == [0.5, 2.0, 1.0]


def test_rows_at_ratio_one_are_bit_copies(dev):
    """In a batch whose other rows are resampled; zeros past the end of the input.  The next f32 above 1 is not a copy."""
    T_in, off = 600, 5
    x = torch.from_numpy(uniform_rows(5, T_in, 22)).to(dev)
    ratio = torch.tensor([1.06, 1.0, 0.94, 1.0, float(np.nextafter(np.float32(1), np.float32(2)))], device=dev)
    got = ops.speed_change(x, ratio, T_OUT, x_offset=off)
    want = torch.zeros(T_OUT, device=dev)
    for b in (1, 3):
        want.zero_()
        want[:T_in - off] = x[b, off:]
        assert torch.equal(got[b].view(torch.int32), want.view(torch.int32))
    for b in (0, 2, 4):
        assert not torch.equal(got[b, :T_in - off], x[b, off:])
    assert float((got[4, :T_in - off - 8] - x[4, off:-8]).abs().max()) > 1e-3        # the 0.99 roll-off is not the identity


def test_one_long_row_keeps_its_position(dev):
    """The position arithmetic: the last 4096 outputs of 300 000 input samples.  An f32 m * rho is off by 0.01 sample
    there, an error of 1e-2 in the output."""
    T_in = 300000
    x = uniform_rows(2, T_in, 23)
    ratios = np.array([1.06, 0.94], dtype=np.float32)
    n_out = [int(np.floor(T_in / float(r))) for r in ratios]
    got = ops.speed_change(torch.from_numpy(x).to(dev), torch.from_numpy(ratios).to(dev), max(n_out), x_offset=0)
    for b in range(2):
        r64, r32 = batch_refs(x[b:b + 1], ratios[b:b + 1], n_out[b], 0, m_from=n_out[b] - 4096)
        _check(f"long row rho={ratios[b]}", got[b:b + 1, n_out[b] - 4096:n_out[b]], r64, r32)


def test_two_launches_give_the_same_bits(dev, small):
    x, off, _ = small["inside"]
    xd, ratio = torch.from_numpy(x).to(dev), torch.from_numpy(SMALL_RATIOS).to(dev)
    a = ops.speed_change(xd, ratio, T_OUT, x_offset=off)
    b = ops.speed_change(xd, ratio, T_OUT, x_offset=off)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_captured_launch_reads_the_ratios_at_replay(dev, small):
    x, off, _ = small["inside"]
    xd = torch.from_numpy(x).to(dev)
    sets = [torch.from_numpy(SMALL_RATIOS).to(dev), torch.tensor([1.0, 1.03, 2.0, 0.7, 0.97, 1.0], device=dev),
            torch.tensor([1.5, 0.5, 1.0, 1.0, float("nan"), 0.99], device=dev)]
    eager = [ops.speed_change(xd, r, T_OUT, x_offset=off) for r in sets]
    ratio, out = sets[0].clone(), torch.empty((6, T_OUT), device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.speed_change(xd, ratio, T_OUT, x_offset=off, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.speed_change(xd, ratio, T_OUT, x_offset=off, out=out)
    for r, want in zip(sets[1:] + sets[:1], eager[1:] + eager[:1]):
        ratio.copy_(r)
        out.fill_(-1.0)
        graph.replay()
        assert torch.equal(out, want)


# ---- the second view's transform ---------------------------------------------------------------------------------
def test_transform_off_is_the_module_without_the_keys(dev):
    x_i, x_j = synthetic_batch(8, 5, dev)
    outs = []
    for extra in ({}, {"speed_prob": 0.0, "speed_range": [0.94, 1.06]}):
        t = GPUTransformNeuralfp(_cfg(**extra), None, _noise_bank(), train=True).to(dev)
        torch.manual_seed(77)
        X = t(x_i, x_j)
        outs.append((X[0], X[1], torch.cuda.get_rng_state(dev)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][2], outs[1][2])
    assert not torch.equal(outs[0][1], t.logmelspec(x_j))                 # the noise was mixed in: draws were made


def test_transform_with_a_fixed_ratio_is_speed_change_then_logmel(dev):
    t = GPUTransformNeuralfp(_cfg(speed_prob=1.0, speed_range=[1.06, 1.06]), None, None, train=True).to(dev)
    pad, clip = t.pad, t.clip
    assert (pad, clip, t.draw_len) == (8, 16000, 16976)
    x_i, x_j = _views(4, t.draw_len, dev)
    X_i, X_j = t(x_i, x_j)
    c = t.cfg
    mel = lambda w: ops.logmel(w, c["fs"], c["n_fft"], c["win_len"], c["hop_len"], c["n_mels"])
    assert torch.equal(X_j, mel(ops.speed_change(x_j, 1.06, clip, pad)))
    assert torch.equal(X_i, mel(x_i[:, pad:pad + clip]))
    assert not torch.equal(X_j, mel(x_j[:, pad:pad + clip]))


def test_transform_with_the_range_one_one_equals_off_on_the_cut_views(dev):
    on = GPUTransformNeuralfp(_cfg(speed_prob=1.0, speed_range=[1.0, 1.0]), None, _noise_bank(), train=True).to(dev)
    off = GPUTransformNeuralfp(_cfg(), None, _noise_bank(), train=True).to(dev)
    x_i, x_j = _views(4, on.draw_len, dev)
    cut = slice(on.pad, on.pad + on.clip)
    torch.manual_seed(3)
    a = on(x_i, x_j)
    torch.manual_seed(3)
    torch.rand(4, device=dev), torch.rand(4, device=dev)                  # the two speed draws `on` made first
    b = off(x_i[:, cut], x_j[:, cut])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_transform_aug_seed_repeats_the_ratios(dev):
    x_i, x_j = _views(6, 16976, dev)
    outs = [GPUTransformNeuralfp(_cfg(speed_prob=0.8, speed_range=[0.94, 1.06], aug_seed=s), None, None, train=True)
            .to(dev)(x_i, x_j)[1] for s in (9, 9, 10)]
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


def test_transform_keeps_about_speed_prob_of_the_clips(dev):
    """4 096 clips at speed_prob = 0.5: the kept share is within 0.5 +- 0.04, five standard deviations of a fair draw.
    A clip that was not kept is the copy of its cut."""
    t = GPUTransformNeuralfp(_cfg(dur=0.1, speed_prob=0.5, speed_range=[0.94, 1.06]), None, None, train=True).to(dev)
    assert t.clip == 1600
    x = torch.from_numpy(uniform_rows(4096, t.draw_len, 24)).to(dev)
    y = t.speed_change(x)
    kept = (y != x[:, t.pad:t.pad + t.clip]).any(dim=1).float().mean().item()
    print(f"kept share {kept:.4f}")
    assert abs(kept - 0.5) <= 0.04


# ---- the corpus draw -----------------------------------------------------------------------------------------------
def test_corpus_draws_both_views_at_draw_len(dev):
    cfg = _cfg(speed_prob=0.7, speed_range=[0.94, 1.06])
    fs = cfg["fs"]
    draw_len = ops.speed_input_len(int(fs * cfg["dur"]), 1.06)
    om_old, om = int(fs * cfg["offset"] + int(fs * cfg["dur"])), int(fs * cfg["offset"]) + draw_len
    assert (draw_len, om_old, om) == (16976, 16800, 17776)
    # track 2 lies between the old and the new eligibility bound; track 4 is one sample short of the new one
    tracks = _tracks([30000, 25000, 17000, 41000, om, om + 1], 41)
    corpus = data.DeviceAudioCorpus(cfg, [t.numpy() for t in tracks], dev)
    assert corpus.draw_len == draw_len and corpus.offset_mod == om and corpus.clip == 16000
    assert corpus.eligible == [0, 1, 3, 5] and corpus.stats["excluded"] == 2
    plain = data.DeviceAudioCorpus(_cfg(), [t.numpy() for t in tracks], dev)
    assert plain.eligible == [0, 1, 2, 3, 4, 5] and plain.stats["excluded"] == 0
    with pytest.raises(ValueError, match="excluded"):
        corpus.draw_pairs([2])
    B, A = 16, 3
    rows = torch.arange(B) % 4
    u = torch.rand((B, A, 3), generator=torch.Generator().manual_seed(42))
    x_i, x_j = ops.draw_pairs(corpus.bank, corpus._el_start, corpus._el_len, corpus._el_norm, rows.to(dev), u.to(dev),
                              corpus.draw_len, corpus.offset_mod, cfg["silence"], corpus._silent)
    ri, rj, _ = draw_pairs_ref([corpus.track(i).cpu() for i in corpus.eligible], corpus._el_norm.cpu(), rows, u, draw_len, om,
                               cfg["silence"])
    assert x_i.shape == (B, draw_len) and torch.equal(x_i.cpu(), ri) and torch.equal(x_j.cpu(), rj)
    # the corpus's own draw: the same uniforms from a seeded generator, through DeviceAudioCorpus.draw_pairs
    ids = [0, 1, 3, 5, 5, 0]
    gen = torch.Generator().manual_seed(43)
    a_i, a_j = corpus.draw_pairs(ids, generator=gen)
    u = torch.rand((len(ids), 8, 3), generator=torch.Generator().manual_seed(43))
    ri, rj, _ = draw_pairs_ref([corpus.track(i).cpu() for i in corpus.eligible], corpus._el_norm.cpu(),
                               torch.tensor([corpus._pos[i] for i in ids]), u, draw_len, om, cfg["silence"])
    assert torch.equal(a_i.cpu(), ri) and torch.equal(a_j.cpu(), rj)
    # what the corpus draws is what the transform takes
    t = GPUTransformNeuralfp(cfg, None, None, train=True).to(dev)
    X_i, X_j = t(a_i, a_j)
    assert X_i.shape == X_j.shape == (len(ids), cfg["n_mels"], 32)


def test_corpus_with_speed_off_draws_what_it_drew(dev):
    tracks = _tracks([30000, 25000, 17000, 41000], 44)
    ids = [0, 1, 2, 3, 2]
    draws = []
    for extra in ({}, {"speed_prob": 0, "speed_range": [0.94, 1.06]}):
        corpus = data.DeviceAudioCorpus(_cfg(**extra), [t.numpy() for t in tracks], dev)
        assert corpus.draw_len == corpus.clip == 16000 and corpus.offset_mod == 16800 and corpus.stats["excluded"] == 0
        draws.append(corpus.draw_pairs(ids, generator=torch.Generator().manual_seed(45)))
    assert draws[0][0].shape == (5, 16000)
    assert torch.equal(draws[0][0], draws[1][0]) and torch.equal(draws[0][1], draws[1][1])


def test_corpus_refuses_a_window_beyond_the_draw_kernel_and_names_speed_range(dev):
    with pytest.raises(ValueError, match="speed_range"):
        data.DeviceAudioCorpus(_cfg(dur=1.3, speed_prob=0.5, speed_range=[1.0, 2.0]), [np.zeros(90000, np.float32)], dev)


# ---- the trainer -----------------------------------------------------------------------------------------------------
def test_trainer_steps_eager_and_graph_with_speed_on(dev):
    cfg = _cfg(speed_prob=0.8, speed_range=[0.94, 1.06])
    torch.manual_seed(0)
    tr = Trainer(cfg, build_model(cfg, device=dev), dev, amp_dtype=torch.bfloat16)
    assert tr.draw_len == 16976
    x_i, x_j = _views(8, tr.draw_len, dev)
    losses = [tr.step(x_i, x_j) for _ in range(2)] + [tr.step_graph(x_i, x_j) for _ in range(3)]
    losses = torch.stack(losses).cpu()
    print("losses", losses.tolist())
    assert bool(torch.isfinite(losses).all())
    assert len(set(losses[2:].tolist())) > 1                  # every replay drew its own ratios and took its own step
    with pytest.raises(ValueError, match="draw_len"):
        tr.step(x_i[:, :16000], x_j[:, :16000])
    with pytest.raises(ValueError):
        tr.step_graph(x_i[:, :16000], x_j[:, :16000])


def test_trainer_at_ratio_one_takes_the_step_of_a_trainer_without_the_keys(dev):
    cfg_on = _cfg(speed_prob=1.0, speed_range=[1.0, 1.0])
    draw_len, pad = ops.speed_input_len(16000, 1.0), ops.speed_pad(1.0)
    x_i, x_j = _views(8, draw_len, dev)
    losses = []
    for cfg, cut in ((cfg_on, slice(None)), (_cfg(), slice(pad, pad + 16000))):
        torch.manual_seed(0)
        tr = Trainer(cfg, build_model(cfg, device=dev), dev, amp_dtype=torch.bfloat16)
        assert tr.draw_len == (draw_len if cfg is cfg_on else 16000)
        losses.append(tr.step(x_i[:, cut], x_j[:, cut]))
    assert torch.equal(losses[0], losses[1]) and bool(torch.isfinite(losses[0]))


# ---- what the augmentation buys ----------------------------------------------------------------------------------------
@pytest.mark.statistical
def test_top1_of_models_trained_with_and_without_speed_augmentation():
    """Two models from the same initial weights, 40 steps each as _retrieval_case.build_case trains (24 + 24 synthetic
    tracks, lr 2e-4, bf16, white noise at 5 dB on the second view): one plain, one with speed_prob = 1 and speed_range =
    [0.94, 1.06].  Then the protocol of test_top1_of_a_trained_model_with_and_without_tempo_at_10db: 60 crops of 9 s per rho
    in 0.96, 1.0, 1.04 at 10 dB, speed changed through fs = round(16000 * rho), identify with and without tempo = 0.06.
    Gated only on what holds for any model: finite losses, and the top-1 score with tempo never below the one without.
    The figures are printed (tools/speed_aug_probe.py runs the same experiment at any number of steps; DESIGN.md section
    12.23 records them)."""
    from tools.speed_aug_probe import experiment
    res = experiment(40, torch.device("cuda:0"))
    for name in ("plain", "speed"):
        assert res[name]["losses_finite"], name
        assert len(res[name]["rows"]) == 3
        for row in res[name]["rows"]:
            assert row["tempo_below_dense"] == 0, (name, row)
