"""Time-stretch augmentation on the MI355X: grafp_time_stretch_f32 against the float64 rule (tests/_stretch_ref.py), the
transform's cfg keys, the corpus draw at draw_len, and the trainer in eager and graph form.

An arg-max cannot be held to a tolerance, so the shifts are checked along the kernel's own path (check_shifts): each
delta_i within the frame's f32 dot-product bound 2 N 2^-24 max sum |t| |x| of the best candidate, and equal to the rule's
winner where that winner leads by more than the bound.  tests/test_stretch_cpu.py shows that on every input here but the
tie case every frame is so certified on the rule's own path: the tests therefore also demand shifts equal to the rule's.

Error bar of the output, given equal shifts: e32 = the largest |stretch_f32 - stretch_f64| over the test's own inputs,
computed on the CPU; the kernel must stay within 8 * e32 of stretch_f64 (about 1e-7 on input of peak 1; the factor covers
the device's sinf / cosf against numpy's, as in tests/test_gpu_speed.py).  A frame spliced one sample off is 1e-2 or more."""
import numpy as np
import pytest
import torch

from _stretch_ref import (LONG_RATIOS, LONG_TAIL, SMALL_RATIOS, T_SMALL, check_shifts, clamp_ratio, frames, long_case,
                          small_cases, stretch_f32, stretch_f64, tie_case)
from _warp_views import _cfg, _noise_bank, _tracks, _views
from grafp_amd import data, ops
from grafp_amd.modules.transformations import GPUTransformNeuralfp
from grafp_amd.train import Trainer, build_model, synthetic_batch

pytestmark = pytest.mark.gpu
NF = frames(T_SMALL)                   # 7


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _check_output(name, got, r64, r32):
    e32 = float(np.abs(r32.astype(np.float64) - r64).max())
    err = float(np.abs(got.double().cpu().numpy() - r64).max())
    print(f"{name}: e32 = {e32:.3e}, kernel error = {err:.3e} ({err / e32:.2f} e32)")
    assert e32 > 0 and err <= 8 * e32, (name, err, e32)


def _check_batch(name, x, ratios, off, refs, got, shifts):
    """Shifts on the kernel's path, shifts against the rule's own, and the outputs of all rows against one e32."""
    shifts = shifts.cpu().numpy()
    for b, ref in enumerate(refs):
        check_shifts(x[b], float(clamp_ratio(ratios[b])), T_SMALL, off, shifts[b])
        assert np.array_equal(shifts[b], ref.shifts), (name, b, shifts[b], ref.shifts)
    r64 = np.stack([ref.out for ref in refs])
    r32 = np.stack([stretch_f32(x[b], ratios[b], T_SMALL, off, refs[b].shifts) for b in range(len(refs))])
    _check_output(name, got, r64, r32)


# ---- the kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("inside", "edges"))
def test_small_shapes_against_the_rule(dev, which):
    x, off, refs = small_cases()[which]
    xd, ratio = torch.tensor(x, device=dev), torch.from_numpy(SMALL_RATIOS).to(dev)
    got, shifts = ops.time_stretch(xd, ratio, T_SMALL, x_offset=off, return_shifts=True)
    assert got.shape == (6, T_SMALL) and got.dtype == torch.float32
    assert shifts.shape == (6, NF) and shifts.dtype == torch.int32
    print(f"{which}: shifts {shifts.cpu().tolist()}")
    _check_batch(which, x, SMALL_RATIOS, off, refs, got, shifts)
    if which == "edges":
        assert refs[5].out[800:].max() == 0 and torch.count_nonzero(got[5, 800:]) == 0      # rho = 2: past the input
        assert torch.count_nonzero(got[5, :400]) > 250
    # without the shifts: one tensor, the same bits
    plain = ops.time_stretch(xd, ratio, T_SMALL, x_offset=off)
    assert torch.is_tensor(plain) and torch.equal(plain.view(torch.int32), got.view(torch.int32))
    # a single clip, 1-D in and out
    one, s1 = ops.time_stretch(xd[4], ratio[4:5], T_SMALL, x_offset=off, return_shifts=True)
    assert one.shape == (T_SMALL,) and s1.shape == (NF,) and torch.equal(one, got[4]) and torch.equal(s1, shifts[4])
    assert torch.equal(ops.time_stretch(xd[4], float(SMALL_RATIOS[4]), T_SMALL, x_offset=off), got[4])


def test_exact_ties_follow_the_rule(dev):
    """Integer input of period 64: every correlation is exact in f32 in any order and candidates 64 apart tie bit for
    bit, so the shifts are the rule's tie-break or the kernel's arg-max is wrong."""
    x, off, T_out, refs = tie_case()
    xd = torch.tensor(np.stack([x, x]), device=dev)
    got, shifts = ops.time_stretch(xd, torch.tensor([0.94, 1.06], device=dev), T_out, x_offset=off, return_shifts=True)
    for b, ref in enumerate(refs):
        print(f"ties row {b}: {shifts[b].cpu().tolist()}")
        assert np.array_equal(shifts[b].cpu().numpy(), ref.shifts)
    r64 = np.stack([r.out for r in refs])
    r32 = np.stack([stretch_f32(x, r, T_out, off, ref.shifts) for r, ref in zip((0.94, 1.06), refs)])
    _check_output("ties", got, r64, r32)


def test_strided_rows_in_and_out(dev):
    x, off, refs = small_cases()["inside"]
    T_in = x.shape[1]
    wide = torch.full((6, T_in + 37), float("nan"), device=dev)
    wide[:, 5:5 + T_in] = torch.tensor(x, device=dev)
    out = torch.full((6, T_SMALL + 11), -7.0, device=dev)
    ratio = torch.from_numpy(SMALL_RATIOS).to(dev)
    ret, shifts = ops.time_stretch(wide[:, 5:5 + T_in], ratio, T_SMALL, x_offset=off, out=out[:, 3:3 + T_SMALL], return_shifts=True)
    assert ret.data_ptr() == out[:, 3:].data_ptr()
    want, want_s = ops.time_stretch(torch.tensor(x, device=dev), ratio, T_SMALL, x_offset=off, return_shifts=True)
    assert torch.equal(ret, want) and torch.equal(shifts, want_s)
    assert bool((out[:, :3] == -7.0).all()) and bool((out[:, 3 + T_SMALL:] == -7.0).all())      # nothing outside the rows
    assert bool(wide[:, :5].isnan().all()) and bool(wide[:, 5 + T_in:].isnan().all())
    _check_batch("strided", x, SMALL_RATIOS, off, refs, ret, shifts)


def test_ratios_are_clamped_and_nan_is_one(dev):
    x, off, _ = small_cases()["inside"]
    xd = torch.tensor(x[:3], device=dev)
    run = lambda r: ops.time_stretch(xd[:len(r)], torch.tensor(r, device=dev), T_SMALL, x_offset=off, return_shifts=True)
    odd, plain, more = run([0.3, 3.0, float("nan")]), run([0.5, 2.0, 1.0]), run([float("-inf"), float("inf"), -1.0])
    assert torch.equal(odd[0], plain[0]) and torch.equal(odd[1], plain[1])
    assert torch.equal(more[0][:2], plain[0][:2]) and torch.equal(more[1][:2], plain[1][:2])
    low = ops.time_stretch(xd[2], torch.tensor([0.5], device=dev), T_SMALL, x_offset=off)
    assert torch.equal(more[0][2], low)
    assert [float(clamp_ratio(r)) for r in (0.3, 3.0, float("nan"))] == [0.5, 2.0, 1.0]
    for b, r in enumerate((0.5, 2.0)):                                     # and the clamped rows follow the rule
        check_shifts(x[b], r, T_SMALL, off, odd[1][b].cpu().numpy())


def test_rows_at_ratio_one_are_bit_copies(dev):
    """In a batch whose other rows are stretched; zeros past the end of the input; all-zero shifts.  The next f32 above 1
    is not a copy: its window sum is 1 only to rounding."""
    x, _, _ = small_cases()["inside"]
    T_in, off = 1200, 5
    xd = torch.from_numpy(x[:5, :T_in].copy()).to(dev)
    ratio = torch.tensor([1.06, 1.0, 0.94, 1.0, float(np.nextafter(np.float32(1), np.float32(2)))], device=dev)
    got, shifts = ops.time_stretch(xd, ratio, T_SMALL, x_offset=off, return_shifts=True)
    want = torch.zeros(T_SMALL, device=dev)
    for b in (1, 3):
        want.zero_()
        want[:T_in - off] = xd[b, off:]
        assert torch.equal(got[b].view(torch.int32), want.view(torch.int32))
        assert int(shifts[b].abs().max()) == 0
    for b in (0, 2, 4):
        assert not torch.equal(got[b, :T_in - off], xd[b, off:])
    assert int(shifts[0].abs().max()) > 0 and int(shifts[2].abs().max()) > 0


def test_one_long_row_keeps_its_position(dev):
    """The position arithmetic: the last frames of 300 000 input samples (the last 16 at 1.06 and 0.94; the last 160 at
    0.97, where an f32 (i - 1) * HS * rho rounds to the other side six times), with the kernel's own shifts fed to the
    reference.  A frame taken one sample off moves its correlations and its output by 1e-2 or more."""
    x, T_out, refs = long_case()
    got, shifts = ops.time_stretch(torch.tensor(x, device=dev), torch.from_numpy(LONG_RATIOS).to(dev), max(T_out),
                                   x_offset=0, return_shifts=True)
    for b, ref in enumerate(refs):
        F = frames(T_out[b])
        first = F - LONG_TAIL[b]
        s = shifts[b, :F].cpu().numpy()
        on_path = check_shifts(x[b], float(LONG_RATIOS[b]), T_out[b], 0, s, first=first)
        assert np.array_equal(s, ref.shifts), (b, np.flatnonzero(s != ref.shifts)[:5])          # the whole path
        lo = (first - 1) * 256
        r32 = stretch_f32(x[b], LONG_RATIOS[b], T_out[b], 0, s, first=first)
        _check_output(f"long row rho={LONG_RATIOS[b]}", got[b, lo:T_out[b]], on_path.out[lo:], r32[lo:])


def test_two_launches_give_the_same_bits(dev):
    x, off, _ = small_cases()["inside"]
    xd, ratio = torch.tensor(x, device=dev), torch.from_numpy(SMALL_RATIOS).to(dev)
    a = ops.time_stretch(xd, ratio, T_SMALL, x_offset=off, return_shifts=True)
    b = ops.time_stretch(xd, ratio, T_SMALL, x_offset=off, return_shifts=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_captured_launch_reads_the_ratios_at_replay(dev):
    x, off, _ = small_cases()["inside"]
    xd = torch.tensor(x, device=dev)
    sets = [torch.from_numpy(SMALL_RATIOS).to(dev), torch.tensor([1.0, 1.03, 2.0, 0.7, 0.97, 1.0], device=dev),
            torch.tensor([1.5, 0.5, 1.0, 1.0, float("nan"), 0.99], device=dev)]
    eager = [ops.time_stretch(xd, r, T_SMALL, x_offset=off) for r in sets]
    ratio, out = sets[0].clone(), torch.empty((6, T_SMALL), device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.time_stretch(xd, ratio, T_SMALL, x_offset=off, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.time_stretch(xd, ratio, T_SMALL, x_offset=off, out=out)
    for r, want in zip(sets[1:] + sets[:1], eager[1:] + eager[:1]):
        ratio.copy_(r)
        out.fill_(-1.0)
        graph.replay()
        assert torch.equal(out, want)


# ---- the second view's transform ---------------------------------------------------------------------------------
STRETCH = {"stretch_prob": 1.0, "stretch_range": [0.94, 1.06]}
SPEED = {"speed_prob": 1.0, "speed_range": [0.94, 1.06]}


def test_transform_off_is_the_module_without_the_keys(dev):
    x_i, x_j = synthetic_batch(8, 5, dev)
    outs = []
    for extra in ({}, {"stretch_prob": 0.0, "stretch_range": [0.94, 1.06]}):
        t = GPUTransformNeuralfp(_cfg(**extra), None, _noise_bank(), train=True).to(dev)
        torch.manual_seed(77)
        X = t(x_i, x_j)
        outs.append((X[0], X[1], torch.cuda.get_rng_state(dev)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][2], outs[1][2])
    assert not torch.equal(outs[0][1], t.logmelspec(x_j))                 # the noise was mixed in: draws were made


def test_transform_with_a_fixed_ratio_is_time_stretch_then_logmel(dev):
    t = GPUTransformNeuralfp(_cfg(stretch_prob=1.0, stretch_range=[1.06, 1.06]), None, None, train=True).to(dev)
    pad, clip = t.pad, t.clip
    assert (pad, clip, t.draw_len) == (401, 16000, 17867)
    x_i, x_j = _views(4, t.draw_len, dev)
    X_i, X_j = t(x_i, x_j)
    assert X_i.shape == X_j.shape == (4, t.cfg["n_mels"], 32)
    c = t.cfg
    mel = lambda w: ops.logmel(w, c["fs"], c["n_fft"], c["win_len"], c["hop_len"], c["n_mels"])
    assert torch.equal(X_j, mel(ops.time_stretch(x_j, 1.06, clip, pad)))
    assert torch.equal(X_i, mel(x_i[:, pad:pad + clip]))
    assert not torch.equal(X_j, mel(x_j[:, pad:pad + clip]))


def test_transform_draws_stretch_before_speed_and_the_chain_is_stretch_speed_noise(dev):
    """Both on with a noise bank: the draws are keep, rho of the stretch, then keep, rho of the speed change, then the
    noise chain's, all from one generator; the result is the three ops applied in that order."""
    cfg = _cfg(stretch_prob=0.5, stretch_range=[0.94, 1.06], speed_prob=0.5, speed_range=[0.9, 1.1])
    t = GPUTransformNeuralfp(cfg, None, _noise_bank(), train=True).to(dev)
    B = 6
    x_i, x_j = _views(B, t.draw_len, dev)
    torch.manual_seed(5)
    got = t(x_i, x_j)[1]
    torch.manual_seed(5)
    one = torch.ones(B, device=dev)
    keep, u = torch.rand(B, device=dev) < 0.5, torch.rand(B, device=dev)
    y = ops.time_stretch(x_j, torch.where(keep, 0.94 + (1.06 - 0.94) * u, one), t.speed_len, x_offset=t.stretch_pad)
    keep, u = torch.rand(B, device=dev) < 0.5, torch.rand(B, device=dev)
    y = ops.speed_change(y, torch.where(keep, 0.9 + (1.1 - 0.9) * u, one), t.clip, x_offset=t.speed_pad)
    want = t.logmelspec(t.augment(y, cfg["ir_prob"], cfg["noise_prob"], cfg["tr_snr"]))
    assert got.shape == (B, cfg["n_mels"], 32) and torch.equal(got, want)


def test_both_augmentations_at_ratio_one_give_equal_views(dev):
    """draw_len = stretch_input_len(speed_input_len(clip, hi), hi) and x_i cut at stretch_pad + speed_pad: at both ratios
    1 the second view is, bit for bit, the first."""
    t = GPUTransformNeuralfp(_cfg(stretch_prob=1.0, stretch_range=[1.0, 1.0], speed_prob=1.0, speed_range=[1.0, 1.0]),
                             None, None, train=True).to(dev)
    assert t.pad == ops.stretch_pad(1.0) + ops.speed_pad(1.0) == 385 + 8
    assert t.draw_len == ops.stretch_input_len(ops.speed_input_len(16000, 1.0), 1.0)
    x = _views(4, t.draw_len, dev)[0]
    X_i, X_j = t(x, x)
    assert torch.equal(X_i.view(torch.int32), X_j.view(torch.int32))
    assert torch.equal(t.train_transform(x).view(torch.int32), x[:, t.pad:t.pad + t.clip].view(torch.int32))
    # and at the ends of a real range both stay inside the drawn samples: a NaN planted outside never shows
    t = GPUTransformNeuralfp(_cfg(**STRETCH, **SPEED), None, None, train=True).to(dev)
    assert t.draw_len == 18952
    wide = torch.full((4, t.draw_len + 2), float("nan"), device=dev)
    wide[:, 1:-1] = _views(4, t.draw_len, dev)[0]
    for rs, rv in ((1.06, 1.06), (0.94, 1.06), (1.06, 0.94), (0.94, 0.94)):
        y = ops.time_stretch(wide[:, 1:-1], rs, t.speed_len, x_offset=t.stretch_pad)
        y = ops.speed_change(y, rv, t.clip, x_offset=t.speed_pad)
        assert bool(torch.isfinite(y).all())


def test_transform_aug_seed_repeats_the_ratios(dev):
    x_i, x_j = _views(6, 17867, dev)
    outs = [GPUTransformNeuralfp(_cfg(stretch_prob=0.8, stretch_range=[0.94, 1.06], aug_seed=s), None, None, train=True)
            .to(dev)(x_i, x_j)[1] for s in (9, 9, 10)]
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


# ---- the corpus draw -----------------------------------------------------------------------------------------------
def test_corpus_draws_both_views_at_draw_len(dev):
    cfg = _cfg(stretch_prob=0.7, stretch_range=[0.94, 1.06])
    fs = cfg["fs"]
    draw_len = ops.stretch_input_len(int(fs * cfg["dur"]), 1.06)
    om = int(fs * cfg["offset"]) + draw_len
    assert (draw_len, om) == (17867, 18667)
    # track 2 lies between the old and the new eligibility bound; track 4 is one sample short of the new one
    tracks = _tracks([30000, 25000, 17000, 41000, om, om + 1], 41)
    corpus = data.DeviceAudioCorpus(cfg, [t.numpy() for t in tracks], dev)
    assert corpus.draw_len == draw_len and corpus.offset_mod == om and corpus.clip == 16000
    assert corpus.eligible == [0, 1, 3, 5] and corpus.stats["excluded"] == 2
    ids = [0, 1, 3, 5, 5, 0]
    a_i, a_j = corpus.draw_pairs(ids, generator=torch.Generator().manual_seed(43))
    assert a_i.shape == a_j.shape == (len(ids), draw_len)
    t = GPUTransformNeuralfp(cfg, None, None, train=True).to(dev)           # what the corpus draws is what the transform takes
    X_i, X_j = t(a_i, a_j)
    assert X_i.shape == X_j.shape == (len(ids), cfg["n_mels"], 32)
    both = data.DeviceAudioCorpus(_cfg(**STRETCH, **SPEED), [t.numpy() for t in tracks], dev)
    assert both.draw_len == 18952 and both.offset_mod == 18952 + 800
    assert both.draw_len == GPUTransformNeuralfp(_cfg(**STRETCH, **SPEED), None, None, train=True).draw_len


def test_corpus_with_stretch_off_draws_what_it_drew(dev):
    tracks = _tracks([30000, 25000, 17000, 41000], 44)
    ids = [0, 1, 2, 3, 2]
    draws = []
    for extra in ({}, {"stretch_prob": 0, "stretch_range": [0.94, 1.06]}):
        corpus = data.DeviceAudioCorpus(_cfg(**extra), [t.numpy() for t in tracks], dev)
        assert corpus.draw_len == corpus.clip == 16000 and corpus.offset_mod == 16800 and corpus.stats["excluded"] == 0
        draws.append(corpus.draw_pairs(ids, generator=torch.Generator().manual_seed(45)))
    assert draws[0][0].shape == (5, 16000)
    assert torch.equal(draws[0][0], draws[1][0]) and torch.equal(draws[0][1], draws[1][1])


def test_corpus_refuses_a_window_beyond_the_draw_kernel_and_names_the_key(dev):
    with pytest.raises(ValueError, match="stretch_range"):
        data.DeviceAudioCorpus(_cfg(dur=1.3, stretch_prob=0.5, stretch_range=[1.0, 2.0]), [np.zeros(90000, np.float32)], dev)
    with pytest.raises(ValueError, match="stretch_range.*speed_range"):
        data.DeviceAudioCorpus(_cfg(dur=1.0, stretch_prob=0.5, stretch_range=[1.0, 1.6], speed_prob=0.5, speed_range=[1.0, 1.6]),
                               [np.zeros(90000, np.float32)], dev)


# ---- the trainer -----------------------------------------------------------------------------------------------------
def test_trainer_steps_eager_and_graph_with_stretch_on(dev):
    cfg = _cfg(stretch_prob=0.8, stretch_range=[0.94, 1.06])
    torch.manual_seed(0)
    tr = Trainer(cfg, build_model(cfg, device=dev), dev, amp_dtype=torch.bfloat16)
    assert tr.draw_len == 17867
    x_i, x_j = _views(8, tr.draw_len, dev)
    losses = [tr.step(x_i, x_j) for _ in range(3)] + [tr.step_graph(x_i, x_j) for _ in range(3)]
    losses = torch.stack(losses).cpu()
    print("losses", losses.tolist())
    assert bool(torch.isfinite(losses).all())
    assert len(set(losses[3:].tolist())) > 1                  # every replay drew its own ratios and took its own step
    with pytest.raises(ValueError, match="draw_len"):
        tr.step(x_i[:, :16000], x_j[:, :16000])
    with pytest.raises(ValueError):
        tr.step_graph(x_i[:, :16000], x_j[:, :16000])


def test_trainer_at_ratio_one_takes_the_step_of_a_trainer_without_the_keys(dev):
    cfg_on = _cfg(stretch_prob=1.0, stretch_range=[1.0, 1.0])
    draw_len, pad = ops.stretch_input_len(16000, 1.0), ops.stretch_pad(1.0)
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
def test_top1_of_models_trained_with_and_without_stretch_augmentation():
    """Two models from the same initial weights, 40 steps of 64 pairs each as _retrieval_case.build_case trains (24 + 24
    synthetic tracks, lr 2e-4, bf16, white noise at 5 dB on the second view): one plain, one with stretch_prob = 1 and
    stretch_range = [0.94, 1.06].  Then section 12.23's protocol with time-stretched queries: 60 crops per rho in 0.96,
    1.0, 1.04, made with ops.time_stretch to 9 s, at 10 dB, identify with and without tempo = 0.06.  Gated only on what
    holds for any model: finite losses, and the top-1 score with tempo never below the one without.  The figures are
    printed (tools/stretch_aug_probe.py runs the same experiment at any number of steps; DESIGN.md section 12.27 records
    them)."""
    from tools.stretch_aug_probe import experiment
    res = experiment(40, torch.device("cuda:0"))
    for name in ("plain", "stretch"):
        assert res[name]["losses_finite"], name
        assert len(res[name]["rows"]) == 3
        for row in res[name]["rows"]:
            assert row["tempo_below_dense"] == 0, (name, row)
