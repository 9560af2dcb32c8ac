"""CPU tests of the audio front end's test infrastructure and host plan: the float64 references of _frontend_ref.py
against the f32 torch restatement in oracle/model.py (two independent routes must agree, and their distance is what the
GPU bars are derived from), and ops.mel_filterbank / ops._MelPlan -- host code that runs without a GPU.  Importing
grafp_amd.ops needs the built library (`make -C grafp_amd/csrc`, no GPU required), as test_host_cpu.py does."""
import math

import pytest
import torch

import _frontend_ref as fr


def _cfg(case):
    n_fft, win_len, hop, n_mels = case[1]
    return dict(fs=fr.FS, n_fft=n_fft, win_len=win_len, hop_len=hop, n_mels=n_mels)


# =============================================================== log-mel: the f32 oracle against the f64 reference
@pytest.mark.parametrize("case", fr.LOGMEL_CASES, ids=fr.LOGMEL_IDS)
def test_logmel_f32_oracle_vs_float64(case):
    """Pins logmel_power64 (torch.stft in f32 and in double are separate transforms) and measures c_ref = max |P32 - Pc| / M
    of the f32 torch path: it must stay within fr.C_REF (itself <= 2e-6), from which the GPU tests take c = 16 c_ref.  On
    the two quiet inputs c_ref reads 2.1e-6 and 1.9e-6: at -95 dB one ulp of the f32 dB value is 1.8e-6 in power, which is
    the relative term's to carry, so there the f32 path is held to the all-entries bound with c = c_ref instead.  Also
    checks what keeps the GPU assertions from being vacuous: on noise every entry (of a band that has bins) is loud, on the
    tone at least 5 % are, and the quiet input straddles the clamp."""
    from oracle import model as om
    name, (n_fft, _win, hop, n_mels), B, T, signal = case
    x, p64 = fr.logmel_case_ref(case)
    db32 = om.logmel(torch.from_numpy(x), _cfg(case))
    assert p64.shape == db32.shape == (B, n_mels, 1 + T // hop) and p64.dtype == torch.float64
    e = fr.logmel_errors(db32, p64)
    c_ref = float(e["floor_raw"].max())
    share = float(e["loud"].double().mean())
    loud_db = float(e["db_err"][e["loud"]].max())
    print(f"\n[frontend] logmel {name}: c_ref={c_ref:.2e} loud share={share:.3f} "
          f"f32 torch path on loud entries: {loud_db:.2e} dB")
    assert float(e["floor_excess"].max()) <= fr.C_REF          # the f32 path meets the all-entries bound with c = c_ref
    if signal != "quiet":
        assert c_ref <= fr.C_REF <= 2e-6
        assert loud_db <= fr.DB_BAR / 10          # the reference leaves (at least) nine tenths of the bar to the kernel
    empty = ~(om.mel_filterbank(n_fft // 2 + 1, n_mels, fr.FS) > 0).any(dim=0)
    assert float(e["loud"][:, ~empty].double().mean()) >= fr.min_loud_share(case)
    if signal == "zeros":
        assert float(p64.abs().max()) == 0.0 and bool((db32 == -100.0).all())
    if signal == "quiet":
        clamped = float((p64 < fr.POWER_FLOOR).double().mean())
        assert 0.0 < clamped < 1.0, clamped
    assert bool(empty.any()) == (name == "g256-128bands-empty")
    if bool(empty.any()):
        assert float(p64[:, empty].abs().max()) == 0.0


def test_logmel_power64_against_a_direct_dft():
    """The reference itself, without torch.stft: one frame by an explicit double DFT of the reflect-padded, windowed
    samples (zero-padded window, hop 160)."""
    case = fr.LOGMEL_CASES[fr.LOGMEL_IDS.index("g512-win400-hop160")]
    from oracle import model as om
    x, p64 = fr.logmel_case_ref(case)
    n_fft, win_len, hop, n_mels = case[1]
    xd = torch.from_numpy(x).double()[0]
    T = xd.numel()
    win = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_len) // 2
    n = torch.arange(win_len, dtype=torch.float64)
    win[left:left + win_len] = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / win_len)
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)
    tt = torch.arange(n_fft, dtype=torch.float64)
    ang = -2.0 * math.pi * torch.outer(k, tt) / n_fft
    fb = om.mel_filterbank(n_fft // 2 + 1, n_mels, fr.FS).double()
    for f in (0, 7, T // hop):                                  # reflected at the start, interior, reflected at the end
        p = f * hop + torch.arange(n_fft) - n_fft // 2
        p = torch.where(p < 0, -p, torch.where(p >= T, 2 * (T - 1) - p, p))
        fr_ = xd[p] * win
        power = (torch.cos(ang) @ fr_) ** 2 + (torch.sin(ang) @ fr_) ** 2
        want = power @ fb
        assert float((p64[0, :, f] - want).abs().max()) <= 1e-11 * float(want.max())


# =============================================================== the host plan
@pytest.mark.parametrize("n_freqs,n_mels", [(513, 64), (513, 40), (513, 16), (513, 128), (129, 40), (257, 64),
                                            (1025, 128), (129, 128)])
def test_mel_filterbank_bit_equal_to_the_oracle(n_freqs, n_mels):
    from grafp_amd import ops
    from oracle import model as om
    mine, want = ops.mel_filterbank(n_freqs, n_mels, fr.FS), om.mel_filterbank(n_freqs, n_mels, fr.FS)
    assert mine.dtype == torch.float32 and mine.shape == (n_freqs, n_mels)
    assert torch.equal(mine, want)


@pytest.mark.parametrize("n_fft,win_len,n_mels", [(1024, 1024, 64), (1024, 1024, 40), (1024, 1024, 16), (1024, 1024, 128),
                                                  (1024, 1024, 33), (1024, 400, 64), (256, 256, 40), (512, 512, 64),
                                                  (2048, 2048, 128), (256, 256, 128), (512, 400, 64)])
def test_mel_plan(n_fft, win_len, n_mels):
    """band_lo .. band_hi is exactly the support of each filter (a short band_hi silently drops bins), an empty band is
    lo > hi, the window is the periodic Hann window centred in n_fft, the twiddles are exp(-2 pi i j / n_fft)."""
    from grafp_amd import ops
    from oracle import model as om
    plan = ops._MelPlan("cpu", fr.FS, n_fft, win_len, n_mels)
    nb = n_fft // 2 + 1
    fb = om.mel_filterbank(nb, n_mels, fr.FS)
    assert torch.equal(plan.fb, fb) and plan.fb.is_contiguous()
    assert plan.band_lo.dtype == plan.band_hi.dtype == torch.int32
    lo, hi = plan.band_lo.long(), plan.band_hi.long()
    k = torch.arange(nb).view(nb, 1)
    assert torch.equal(fb > 0, (k >= lo.view(1, -1)) & (k <= hi.view(1, -1)))
    empty = ~(fb > 0).any(dim=0)
    assert torch.equal(lo > hi, empty)
    assert bool(((lo >= 0) & (hi < nb)).all())
    if (n_fft, n_mels) == (256, 128):
        assert int(empty.sum()) >= 1                           # the GPU case with empty bands really has one
    else:
        assert int(empty.sum()) == 0
    # window: double periodic Hann, centred, rounded to f32
    n = torch.arange(win_len, dtype=torch.float64)
    w64 = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_len) // 2
    w64[left:left + win_len] = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / win_len)
    assert plan.window.dtype == torch.float32 and plan.window.shape == (n_fft,)
    assert float((plan.window.double() - w64).abs().max()) <= 2.0 ** -21
    # (torch builds it in f32: two roundings of an angle below 2 pi, 2^-22 each, at slope 1/2, then cos and the result;
    #  a symmetric instead of a periodic window, or one a sample off centre, is wrong by about 1 / win_len)
    assert bool((plan.window[:left] == 0).all()) and bool((plan.window[left + win_len:] == 0).all())
    # twiddles: rounded from double
    j = torch.arange(n_fft // 2, dtype=torch.float64)
    want = torch.stack((torch.cos(2.0 * math.pi * j / n_fft), -torch.sin(2.0 * math.pi * j / n_fft)), dim=1)
    assert plan.twiddle.shape == (n_fft // 2, 2) and plan.twiddle.dtype == torch.float32
    assert torch.equal(plan.twiddle, want.to(torch.float32))


def test_unfold64():
    x = torch.arange(5 * 50, dtype=torch.float32).reshape(5, 50)
    seg = fr.unfold64(x, 8, 13)
    assert seg.shape == (4, 5, 8)
    for s in range(4):
        assert torch.equal(seg[s], x[:, 13 * s:13 * s + 8])
    assert fr.unfold64(x, 51, 1).shape == (0, 5, 51)


# =============================================================== peak extractor: the f32 oracle against the f64 reference
@pytest.mark.parametrize("shape", fr.PEAK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_peak_extract_f32_oracle_vs_float64(shape):
    """Forward inside the project's bar (1e-5 + 1e-4 |.|), ReLU masks equal away from the ambiguous positions, and the
    weight / bias gradients of the masked upstream gradient within a tenth of the GPU bar -- the f32 torch path leaves
    nine tenths of it to the kernels.  Ambiguous positions (|z| < 1e-4) are at most 1e-3 of all."""
    from oracle import model as om
    c = fr.peak_case(shape)
    B, H, W, nf, KH, KW, sh = shape
    Ho = (H + 2 * (KH // 2) - KH) // sh + 1
    assert c["out64"].shape == (B, nf, Ho * W) and c["z"].dtype == torch.float64
    assert torch.equal(c["out64"], torch.clamp(c["z"], min=0.0))
    share = float(c["ambiguous"].double().mean())
    assert share <= 1e-3, share
    assert bool((c["g"][c["ambiguous"]] == 0).all())
    w = c["w"].clone().requires_grad_(True)
    b = c["b"].clone().requires_grad_(True)
    out = om.peak_extract({"peak_extractor.convs.0.weight": w, "peak_extractor.convs.0.bias": b}, c["spec"], sh)
    out.backward(c["g"])
    fwd = fr.forward_excess(out.detach(), c["out64"])
    keep = ~c["ambiguous"]
    assert torch.equal((out.detach() > 0)[keep], (c["z"] > 0)[keep])
    ew, eb = fr.rel_max(w.grad, c["dw64"]), fr.rel_max(b.grad, c["db64"])
    print(f"\n[frontend] peak {shape}: ambiguous share={share:.1e} f32 torch path: forward excess={fwd:.1e} "
          f"dW={ew:.1e} dbias={eb:.1e} (of max)")
    assert fwd <= 0.0
    assert ew <= fr.peak_grad_bar(shape) / 10 and eb <= fr.peak_grad_bar(shape) / 10


def test_peak_extract64_against_explicit_loops():
    """The reference itself, without conv2d: a few outputs of a non-square, strided shape by explicit double sums."""
    shape = (3, 33, 20, 5, 5, 3, 2)
    c = fr.peak_case(shape)
    B, H, W, nf, KH, KW, sh = shape
    spec, w, b = c["spec"].double(), c["w"].double(), c["b"].double()
    t_ramp, f_ramp = torch.linspace(0, 1, W).double(), torch.linspace(0, 1, H).double()
    for (bi, f, y, x) in [(0, 0, 0, 0), (1, 2, 7, 19), (2, 4, 16, 10), (1, 3, 16, 0)]:
        lo, hi = spec[bi].min(), spec[bi].max()
        acc = b[f].clone()
        for ky in range(KH):
            for kx in range(KW):
                yy, xx = y * sh + ky - KH // 2, x + kx - KW // 2
                if 0 <= yy < H and 0 <= xx < W:
                    acc += w[f, 0, ky, kx] * t_ramp[xx] + w[f, 1, ky, kx] * f_ramp[yy] \
                        + w[f, 2, ky, kx] * (spec[bi, yy, xx] - lo) / (hi - lo)
        assert abs(float(c["z"][bi, f, y * W + x] - acc)) <= 1e-12
