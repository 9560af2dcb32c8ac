"""GPU tests of the impulse-response and noise augmentation (grafp_amd/csrc/augment.hip: ir_convolve_kernel,
mix_partial_kernel + mix_apply_kernel) and of the draws that drive it (GPUTransformNeuralfp.augment): every case of
tests/_augment_ref.py against its float64 reference within the derived bar, on every clip, the convolution also bit for bit
against the C oracle; the C entries with row strides wider than the rows; what the C entries and ops refuse before any
launch; the per-clip draws at five standard deviations of a fair draw.  No argument in this file that reaches a kernel lies
outside its bank: every out-of-range one is refused on the host.  `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

import _augment_ref as ar
from _hashfill import hash_normalish

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def _t(a, dev=None):
    t = torch.from_numpy(np.array(a))                       # a copy: the cached cases are read-only
    return t if dev is None else t.to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_ORACLE = {}


def _oracle_conv(name):
    """The C oracle's output of a convolution case, once per process."""
    if name not in _ORACLE:
        from oracle import native as on
        (x, recs, idx), _ = ar.cached_conv(name)
        flat, starts, lens = ar.ragged(recs)
        _ORACLE[name] = on.ir_convolve(x, flat, lens, idx, starts)
    return _ORACLE[name]


def _banks(recs, dev):
    """The two forms of a bank as ops arguments: ragged with HOST tables (their values are checked), padded with DEVICE
    tables (never read back)."""
    flat, starts, lens = ar.ragged(recs)
    return {"ragged": (_t(flat, dev), _t(lens), _t(starts)), "padded": (_t(ar.padded(recs), dev), _t(lens, dev), None)}


# ---- the kernels against the references ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in ar.CONV_CASES])
def test_convolution_within_the_bar_and_equal_to_the_oracle(dev, name):
    """Every output of every convolved clip within gamma(n_t) S[t] of float64 and equal to the oracle's fmaf chain (==: a
    zero-padded tap may flip a zero's sign); the skipped clip is its input, bit for bit.  Ragged and padded bank."""
    from grafp_amd import ops
    (x, recs, idx), _ = ar.cached_conv(name)
    want, on = _oracle_conv(name), idx >= 0
    for form, (bank, lens, starts) in _banks(recs, dev).items():
        index = _t(idx) if form == "ragged" else _t(idx, dev)
        got = ops.ir_convolve(_t(x, dev), bank, lens, index, starts).cpu().numpy()
        ratio = ar.conv_excess(got, name)
        print(f"augment-bar conv {name} {form}: worst error / bar {ratio:.3f}")
        assert ratio <= 1.0, (form, ratio)
        assert np.array_equal(got[on], want[on]), (form, int((got[on] != want[on]).sum()))
        assert np.array_equal(_bits(got[~on]), _bits(x[~on])), form


def test_convolution_without_an_index_with_none_applied_and_on_one_signal(dev):
    """ir_index=None: recording 0 for every clip; all indices negative: a copy; a 1-D x (the validation path): row b of
    the batch, 1-D."""
    from grafp_amd import ops
    from oracle import native as on
    (x, recs, idx), _ = ar.cached_conv("tile-seam")
    bank, lens, starts = _banks(recs, dev)["ragged"]
    xd = _t(x, dev)
    flat, st, ln = ar.ragged(recs)
    got = ops.ir_convolve(xd, bank, lens, None, starts).cpu().numpy()
    assert np.array_equal(got, on.ir_convolve(x, flat, ln, None, st))
    for b in range(x.shape[0]):
        ref, bar = ar.conv_ref(x[b], recs[0])
        assert ar.worst_ratio(np.abs(got[b] - ref), bar) <= 1.0, b
    none = ops.ir_convolve(xd, bank, lens, torch.full((x.shape[0],), -1, dtype=torch.int64), starts)
    assert np.array_equal(_bits(none.cpu().numpy()), _bits(x))
    batch = ops.ir_convolve(xd, bank, lens, _t(idx), starts)
    for b in (2, 4):                                                   # L = 4097 > T, and the skipped clip
        one = ops.ir_convolve(xd[b], bank, lens, _t(idx[b:b + 1]), starts)
        assert one.shape == (x.shape[1],) and torch.equal(one.view(torch.int32), batch[b].view(torch.int32))


@pytest.mark.parametrize("name", [c.name for c in ar.MIX_CASES])
def test_mix_within_the_bar(dev, name):
    """Every sample of every mixed clip within eps_scale |scale n[t]| + u |want[t]| of float64; the skipped clip is its
    input, bit for bit; a zero signal or a zero recording gives the input back, finite.  Ragged and padded bank give the
    same bits."""
    from grafp_amd import ops
    case = ar.MIX_BY_NAME[name]
    (x, recs, idx, off, snr), _ = ar.cached_mix(name)
    seen = {}
    for form, (bank, lens, starts) in _banks(recs, dev).items():
        args = (_t(idx), _t(off), _t(snr)) if form == "ragged" else (_t(idx, dev), _t(off, dev), _t(snr, dev))
        got = seen[form] = ops.mix_snr(_t(x, dev), bank, lens, *args, starts).cpu().numpy()
        assert np.isfinite(got).all()
        ratio = ar.mix_excess(got, name)
        print(f"augment-bar mix {name} {form}: worst error / bar {ratio:.3f}")
        assert ratio <= 1.0, (form, ratio)
        assert np.array_equal(_bits(got[idx < 0]), _bits(x[idx < 0])), form
        if case.kind in ("zero-signal", "zero-noise"):
            assert np.array_equal(got, x), form
    assert np.array_equal(_bits(seen["ragged"]), _bits(seen["padded"]))


def test_mix_on_one_signal(dev):
    """A 1-D x (the validation path) is row b of the batch and comes back 1-D."""
    from grafp_amd import ops
    (x, recs, idx, off, snr), _ = ar.cached_mix("nl-256")
    bank, lens, starts = _banks(recs, dev)["ragged"]
    batch = ops.mix_snr(_t(x, dev), bank, lens, _t(idx), _t(off), _t(snr), starts)
    for b in (2, 4):
        one = ops.mix_snr(_t(x[b], dev), bank, lens, _t(idx[b:b + 1]), _t(off[b:b + 1]), _t(snr[b:b + 1]), starts)
        assert one.shape == (x.shape[1],) and torch.equal(one.view(torch.int32), batch[b].view(torch.int32))


# ---- the C entries: strides and refusals -------------------------------------------------------------------------------
SENTINEL = -777.25


class _Raw:
    """Device tensors of a case and the two C entries on them (grafp_ir_convolve_f32 / grafp_mix_snr_f32), by ctypes."""

    def __init__(self, dev, x, recs, idx, off=None, snr=None):
        from grafp_amd import ops
        self.ops, self.lib = ops, ops.lib
        flat, starts, lens = ar.ragged(recs)
        self.B, self.T, self.n = x.shape[0], x.shape[1], len(recs)
        self.x, self.bank, self.starts, self.lens, self.idx = _t(x, dev), _t(flat, dev), _t(starts, dev), _t(lens, dev), _t(idx, dev)
        self.off = None if off is None else _t(off, dev)
        self.snr = None if snr is None else _t(snr, dev)
        self.need = self.lib.grafp_mix_snr_workspace(self.B, self.T)
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=dev)

    def conv(self, x, x_stride, out, out_stride, n=None):
        p = self.ops._p
        return self.lib.grafp_ir_convolve_f32(p(x), x_stride, self.B, self.T, p(self.bank), p(self.starts), self.n if n is None else n,
                                              p(self.lens), p(self.idx), p(out), out_stride, self.ops._stream())

    def mix(self, x, x_stride, out, out_stride, n=None, ws="own", ws_bytes=None):
        p = self.ops._p
        return self.lib.grafp_mix_snr_f32(p(x), x_stride, self.B, self.T, p(self.bank), p(self.starts), self.n if n is None else n,
                                          p(self.lens), p(self.idx), p(self.off), p(self.snr), p(out), out_stride,
                                          p(self.ws) if ws == "own" else None, self.need if ws_bytes is None else ws_bytes,
                                          self.ops._stream())

    def error(self):
        return self.lib.grafp_last_error()


def _wide(raw, dev):
    """x in a (B, T + 5) buffer (the 5 columns behind a row hold the sentinel) and a (B, T + 3) output full of it."""
    xw = torch.full((raw.B, raw.T + 5), SENTINEL, device=dev)
    xw[:, :raw.T] = raw.x
    return xw, torch.full((raw.B, raw.T + 3), SENTINEL, device=dev)


def test_strides_wider_than_the_rows(dev):
    """x_stride = T + 5 and out_stride = T + 3 at T = 4097 (two tiles / chunks, the last of one sample): the bits of the
    contiguous call, and not one padding column written."""
    (x, recs, idx), _ = ar.cached_conv("tile-seam")
    raw = _Raw(dev, x, recs, idx)
    assert raw.T == 4097
    xw, ow = _wide(raw, dev)
    flat = torch.full((raw.B, raw.T), SENTINEL, device=dev)
    assert raw.conv(raw.x, raw.T, flat, raw.T) == 0, raw.error()
    assert raw.conv(xw, raw.T + 5, ow, raw.T + 3) == 0, raw.error()
    torch.cuda.synchronize()
    assert torch.equal(ow[:, :raw.T].contiguous().view(torch.int32), flat.view(torch.int32))
    assert bool((ow[:, raw.T:] == SENTINEL).all()) and bool((xw[:, raw.T:] == SENTINEL).all())
    assert ar.conv_excess(flat.cpu().numpy(), "tile-seam") <= 1.0

    (x, recs, idx, off, snr), _ = ar.cached_mix("nl-256")
    raw = _Raw(dev, x, recs, idx, off, snr)
    assert raw.T == 4097
    xw, ow = _wide(raw, dev)
    flat = torch.full((raw.B, raw.T), SENTINEL, device=dev)
    assert raw.mix(raw.x, raw.T, flat, raw.T) == 0, raw.error()
    assert raw.mix(xw, raw.T + 5, ow, raw.T + 3) == 0, raw.error()
    torch.cuda.synchronize()
    assert torch.equal(ow[:, :raw.T].contiguous().view(torch.int32), flat.view(torch.int32))
    assert bool((ow[:, raw.T:] == SENTINEL).all()) and bool((xw[:, raw.T:] == SENTINEL).all())
    assert ar.mix_excess(flat.cpu().numpy(), "nl-256") <= 1.0


def test_c_entries_refuse_before_any_launch(dev):
    """Each call returns non-zero with the reason in grafp_last_error, and the output keeps its sentinel: nothing ran."""
    (x, recs, idx), _ = ar.cached_conv("one-thread-8")
    raw = _Raw(dev, x, recs, idx)
    out = torch.full((raw.B, raw.T), SENTINEL, device=dev)
    T = raw.T
    assert raw.conv(raw.x, T, raw.x, T) != 0 and b"ir_convolve: in-place operation is not supported" in raw.error()
    assert raw.conv(raw.x, T - 1, out, T) != 0 and b"ir_convolve: strides shorter than the rows" in raw.error()
    assert raw.conv(raw.x, T, out, T - 1) != 0 and b"ir_convolve: strides shorter than the rows" in raw.error()
    assert raw.conv(raw.x, T, out, T, n=0) != 0 and b"ir_convolve: bad shape" in raw.error() and b"n_ir=0" in raw.error()

    (x, recs, idx, off, snr), _ = ar.cached_mix("nl-2")
    raw = _Raw(dev, x, recs, idx, off, snr)
    out2 = torch.full((raw.B, raw.T), SENTINEL, device=dev)
    T = raw.T
    assert raw.need == raw.B * 8
    assert raw.mix(raw.x, T, out2, T, ws_bytes=raw.need - 1) != 0
    assert f"mix_snr: workspace {raw.need - 1} bytes < required {raw.need}".encode() in raw.error()
    assert raw.mix(raw.x, T, out2, T, ws=None) != 0 and b"mix_snr: workspace" in raw.error()
    assert raw.mix(raw.x, T - 1, out2, T) != 0 and b"mix_snr: strides shorter than the rows" in raw.error()
    assert raw.mix(raw.x, T, out2, T - 1) != 0 and b"mix_snr: strides shorter than the rows" in raw.error()
    assert raw.mix(raw.x, T, out2, T, n=0) != 0 and b"mix_snr: bad shape" in raw.error() and b"n_noise=0" in raw.error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((out2 == SENTINEL).all())


# ---- ops: what the host refuses, and that in-range host tensors pass ---------------------------------------------------------
def _mix_call(dev, **change):
    """Arguments of an ops.mix_snr call on the `nl-2` case (flat bank, host tables), some of them replaced."""
    (x, recs, idx, off, snr), _ = ar.cached_mix("nl-2")
    flat, starts, lens = ar.ragged(recs)
    a = dict(x=_t(x, dev), noise_bank=_t(flat, dev), noise_len=_t(lens), noise_index=_t(idx), noise_offset=_t(off),
             snr_db=_t(snr), noise_start=_t(starts))
    a.update(change)
    return a


def test_ops_refuse_arguments_that_do_not_fit(dev):
    """Every refusal is a ValueError that names the op, raised before anything is launched."""
    from grafp_amd import ops
    a = _mix_call(dev)
    x, bank, lens, idx, off, snr, starts = (a[k] for k in ("x", "noise_bank", "noise_len", "noise_index", "noise_offset",
                                                            "snr_db", "noise_start"))
    B, n, room = x.shape[0], lens.numel(), bank.numel()
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)                                       # noqa: E731
    for name, call in (("ir_convolve", lambda **k: ops.ir_convolve(k["x"], k["noise_bank"], k["noise_len"], k["noise_index"],
                                                                  k["noise_start"])),
                       ("mix_snr", lambda **k: ops.mix_snr(**k))):
        index_name = "noise_index" if name == "mix_snr" else "ir_index"
        bad = [
            (dict(x=x.reshape(B, 1, -1)), r"x must be \(B, T\) or \(T,\)"),
            (dict(x=x[0, 0]), r"x must be \(B, T\) or \(T,\)"),
            (dict(noise_start=None), "a flat bank needs the `starts`"),
            (dict(noise_bank=bank.reshape(1, 1, -1)), "the bank must be a flat buffer"),
            (dict(noise_start=starts[:1]), rf"{n} lengths for 1 recordings"),
            (dict(noise_start=starts[:0], noise_len=lens[:0]), "0 lengths for 0 recordings"),
            (dict(noise_bank=bank[:38].reshape(2, 19), noise_start=None, noise_len=lens[:1]), "1 lengths for 2 recordings"),
            (dict(noise_index=idx[:B - 1]), rf"{B - 1} entries in `{index_name}` for {B} clips"),
            # values of host tensors
            (dict(noise_len=i64(37, 0)), "a length >= 1 and a start >= 0"),
            (dict(noise_start=i64(-1, 37)), "a length >= 1 and a start >= 0"),
            (dict(noise_len=i64(37, 3)), "a recording ends beyond the bank"),
            (dict(noise_start=i64(0, room)), "a recording ends beyond the bank"),
            (dict(noise_bank=bank[:38].reshape(2, 19), noise_start=None, noise_len=i64(19, 20)), "a recording ends beyond the bank"),
            (dict(noise_index=i64(1, 1, n, 1, -1)), rf"must be below the {n} recordings"),
        ]
        if name == "mix_snr":
            bad += [(dict(noise_offset=torch.cat([off, off[:1]])), rf"{B + 1} entries in `noise_offset` for {B} clips"),
                    (dict(snr_db=torch.cat([snr, snr[:1]])), rf"{B + 1} entries in `snr_db` for {B} clips"),
                    (dict(noise_offset=i64(1, 1, -1, 1, 0)), "`noise_offset` must be >= 0"),
                    (dict(noise_offset=i64(1, 1, 2 ** 31, 1, 0)), "`noise_offset` must be >= 0")]
        for change, message in bad:
            with pytest.raises(ValueError, match=rf"^{name}: .*{message}"):
                call(**_mix_call(dev, **change))


def test_ops_take_in_range_host_tensors(dev):
    """Host tables at the edges of what is legal -- the last recording ends with the bank, an index of n - 1, an offset of
    nl - 1 and one beyond nl, int64 and int32 alike -- pass and give the bits of the same call with device tensors."""
    from grafp_amd import ops
    a = _mix_call(dev)
    assert int(a["noise_start"][-1] + a["noise_len"][-1]) == a["noise_bank"].numel() and int(a["noise_index"].max()) == 1
    a["noise_offset"] = torch.tensor([1, 0, 5, 2 ** 31 - 1, 0], dtype=torch.int64)
    on_dev = {k: (v.to(dev) if k != "x" else v) for k, v in a.items()}
    got, want = ops.mix_snr(**a), ops.mix_snr(**on_dev)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    narrow = {k: (v.to(torch.int32) if k in ("noise_index", "noise_offset", "noise_start") else v) for k, v in a.items()}
    assert torch.equal(ops.mix_snr(**narrow).view(torch.int32), want.view(torch.int32))
    conv = lambda k: ops.ir_convolve(k["x"], k["noise_bank"], k["noise_len"], k["noise_index"], k["noise_start"])   # noqa: E731
    assert torch.equal(conv(a).view(torch.int32), conv(on_dev).view(torch.int32))


# ---- the draws of GPUTransformNeuralfp.augment ---------------------------------------------------------------------------------
N_CLIPS, CLIP = 4096, 64
IR_LENS, NOISE_LENS = (1, 3, 17, 64, 100), (1, 7, 64, 300)
IR_PROB, NOISE_PROB = 0.3, 0.8


def _draw_banks():
    irs = [hash_normalish(f"aug:draw.ir{i}", (L,)) / np.sqrt(L) for i, L in enumerate(IR_LENS)]
    noises = [0.3 * hash_normalish(f"aug:draw.noise{i}", (L,)) if L > 1 else np.array([0.25]) for i, L in enumerate(NOISE_LENS)]
    return [a.astype(np.float32) for a in irs], [a.astype(np.float32) for a in noises]


def _transform(dev, irs, noises, train=True, abl=False, **cfg):
    from grafp_amd.modules.transformations import GPUTransformNeuralfp
    from grafp_amd.util import load_config
    return GPUTransformNeuralfp(dict(load_config(), **cfg), irs, noises, train=train, abl=abl).to(dev)


def _capture(monkeypatch):
    """Wrap ops.ir_convolve / ops.mix_snr: they still run; what went in and what came out is kept (host copies)."""
    from grafp_amd import ops
    calls = {"ir": [], "mix": []}
    real_ir, real_mix = ops.ir_convolve, ops.mix_snr
    host = lambda t: t.detach().cpu().numpy().copy()                                          # noqa: E731

    def ir_convolve(x, ir_bank, ir_len, ir_index=None, ir_start=None):
        out = real_ir(x, ir_bank, ir_len, ir_index, ir_start)
        calls["ir"].append(dict(x=host(x), index=host(ir_index), out=host(out)))
        return out

    def mix_snr(x, noise_bank, noise_len, noise_index, noise_offset, snr_db, noise_start=None):
        out = real_mix(x, noise_bank, noise_len, noise_index, noise_offset, snr_db, noise_start)
        calls["mix"].append(dict(x=host(x), index=host(noise_index), offset=host(noise_offset), snr=host(snr_db), out=host(out)))
        return out

    monkeypatch.setattr(ops, "ir_convolve", ir_convolve)
    monkeypatch.setattr(ops, "mix_snr", mix_snr)
    return calls


@pytest.fixture(scope="module")
def clips(dev):
    return _t((0.1 * hash_normalish("aug:draw.x", (N_CLIPS, CLIP))).astype(np.float32), dev)


def _within_5_sigma_of_share(count, total, p):
    """|count / total - p| <= 5 sqrt(p (1 - p) / total): five standard deviations of a binomial share"""
    return abs(count / total - p) <= 5.0 * np.sqrt(p * (1.0 - p) / total)


def test_draws_are_fair(dev, clips, monkeypatch):
    """ir_prob = 0.3, noise_prob = 0.8, tr_snr = [0, 20] on 4096 clips: shares, joint share, picks, offsets and SNR, each at
    five standard deviations of a fair draw (the formula stands at each assertion); skipped clips keep their bits."""
    irs, noises = _draw_banks()
    lo, hi = 0.0, 20.0
    t = _transform(dev, irs, noises, aug_seed=5, ir_prob=IR_PROB, noise_prob=NOISE_PROB, tr_snr=[lo, hi])
    calls = _capture(monkeypatch)
    out = t.train_transform(clips)
    assert len(calls["ir"]) == len(calls["mix"]) == 1
    ir, mix = calls["ir"][0], calls["mix"][0]
    B = N_CLIPS
    assert ir["index"].shape == mix["index"].shape == mix["offset"].shape == mix["snr"].shape == (B,)
    ir_on, mix_on = ir["index"] >= 0, mix["index"] >= 0
    # shares: a binomial share of B draws has standard deviation sqrt(p (1 - p) / B)
    assert _within_5_sigma_of_share(ir_on.sum(), B, IR_PROB), ir_on.mean()
    assert _within_5_sigma_of_share(mix_on.sum(), B, NOISE_PROB), mix_on.mean()
    # independent draws: both apply with probability ir_prob * noise_prob
    assert _within_5_sigma_of_share((ir_on & mix_on).sum(), B, IR_PROB * NOISE_PROB), (ir_on & mix_on).mean()
    # picks: among the n_on applied clips every one of the n recordings has a share of 1 / n
    for what, index, on, n in (("ir", ir["index"], ir_on, len(IR_LENS)), ("noise", mix["index"], mix_on, len(NOISE_LENS))):
        assert index.max() < n and index[~on].tolist() == [-1] * int((~on).sum())
        for r in range(n):
            assert _within_5_sigma_of_share((index[on] == r).sum(), on.sum(), 1.0 / n), (what, r, (index[on] == r).mean())
    # offsets: inside the picked recording (known where the clip is applied), inside the longest one everywhere
    lens = np.array(NOISE_LENS)
    off = mix["offset"]
    assert (off >= 0).all() and (off < lens.max()).all() and (off[mix_on] < lens[mix["index"][mix_on]]).all()
    assert (off[mix_on & (mix["index"] == 0)] == 0).all() and (mix_on & (mix["index"] == 0)).any()      # the length-1 recording
    # SNR: uniform in [lo, hi] has mean (lo + hi) / 2 and standard deviation (hi - lo) / sqrt(12)
    snr = mix["snr"].astype(np.float64)
    assert (snr >= lo).all() and (snr <= hi).all()
    assert abs(snr.mean() - 0.5 * (lo + hi)) <= 5.0 * (hi - lo) / np.sqrt(12.0 * B)
    # skipped clips keep their bits, through each op and through the chain
    x = clips.cpu().numpy()
    assert np.array_equal(_bits(ir["x"]), _bits(x)) and np.array_equal(_bits(mix["x"]), _bits(ir["out"]))
    assert np.array_equal(_bits(ir["out"][~ir_on]), _bits(x[~ir_on]))
    assert np.array_equal(_bits(mix["out"][~mix_on]), _bits(mix["x"][~mix_on]))
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(mix["out"])) and np.array_equal(_bits(got[~ir_on & ~mix_on]), _bits(x[~ir_on & ~mix_on]))
    assert (got[ir_on] != x[ir_on]).any(axis=1).all() and (got[mix_on] != mix["x"][mix_on]).any(axis=1).all()


def test_probabilities_one_and_zero_and_the_offsets_of_every_clip(dev, clips, monkeypatch):
    """ir_prob = noise_prob = 1 applies every clip -- every pick is then visible, so every offset is held to its own
    recording and the 300-sample recording's offsets cover at least 90 % of its positions (1024 draws expected: a fair draw
    leaves 300 exp(-1024 / 300) = 10 positions out) -- and 0 applies none: the output is the input."""
    irs, noises = _draw_banks()
    calls = _capture(monkeypatch)
    _transform(dev, irs, noises, aug_seed=6, ir_prob=1.0, noise_prob=1.0).train_transform(clips)
    ir, mix = calls["ir"][0], calls["mix"][0]
    assert (ir["index"] >= 0).all() and (mix["index"] >= 0).all()
    lens = np.array(NOISE_LENS)
    assert (mix["offset"] >= 0).all() and (mix["offset"] < lens[mix["index"]]).all()
    assert (mix["offset"][mix["index"] == 0] == 0).all()
    for r, L in enumerate(NOISE_LENS):
        assert _within_5_sigma_of_share((mix["index"] == r).sum(), N_CLIPS, 1.0 / len(NOISE_LENS))
    assert np.unique(mix["offset"][mix["index"] == 3]).size >= 0.9 * 300
    assert np.unique(mix["offset"][mix["index"] == 1]).size == 7
    calls["ir"].clear(), calls["mix"].clear()
    out = _transform(dev, irs, noises, aug_seed=6, ir_prob=0.0, noise_prob=0.0).train_transform(clips)
    assert (calls["ir"][0]["index"] == -1).all() and (calls["mix"][0]["index"] == -1).all()
    assert torch.equal(out.view(torch.int32), clips.view(torch.int32))


def test_validation_and_ablation_chains_and_two_seeds(dev, clips, monkeypatch):
    """val_transform applies both transforms to a 1-D track of 3 * 4096 + 5 samples with an SNR inside val_snr; ablation
    leaves the impulse response off and mixes; two seeds draw differently, one seed twice the same."""
    irs, noises = _draw_banks()
    track = clips.reshape(-1)[:3 * 4096 + 5].contiguous()
    calls = _capture(monkeypatch)
    val = _transform(dev, irs, noises, train=False, aug_seed=7, val_snr=[2.0, 4.0])
    out = val.val_transform(track)
    ir, mix = calls["ir"][0], calls["mix"][0]
    assert out.shape == track.shape and ir["x"].shape == mix["x"].shape == (1, track.numel())
    assert 0 <= ir["index"][0] < len(IR_LENS) and 0 <= mix["index"][0] < len(NOISE_LENS)
    assert 2.0 <= mix["snr"][0] <= 4.0 and 0 <= mix["offset"][0] < NOISE_LENS[mix["index"][0]]
    assert not np.array_equal(ir["out"], ir["x"]) and not np.array_equal(mix["out"], mix["x"])
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(mix["out"][0]))
    calls["ir"].clear(), calls["mix"].clear()
    out = val.ablation(track)
    ir, mix = calls["ir"][0], calls["mix"][0]
    assert ir["index"].tolist() == [-1] and np.array_equal(_bits(ir["out"]), _bits(ir["x"]))
    assert mix["index"][0] >= 0 and 2.0 <= mix["snr"][0] <= 4.0 and not np.array_equal(mix["out"], mix["x"])
    draws = []
    for seed in (11, 11, 12):
        calls["ir"].clear(), calls["mix"].clear()
        _transform(dev, irs, noises, aug_seed=seed, ir_prob=IR_PROB, noise_prob=NOISE_PROB).train_transform(clips[:256])
        draws.append((calls["ir"][0]["index"], calls["mix"][0]["index"], calls["mix"][0]["offset"], calls["mix"][0]["snr"]))
    assert all(np.array_equal(a, b) for a, b in zip(draws[0], draws[1]))
    assert not any(np.array_equal(a, b) for a, b in zip(draws[0], draws[2]))


def test_realised_snr_is_the_drawn_one(dev, clips, monkeypatch):
    """A noise-only transform: per applied clip 20 log10(rms(x) / rms(out - x)) in float64 is within 2e-3 dB of the SNR
    that was drawn for it (the bar of test_mix_snr_vs_oracle), whichever recording and offset."""
    _, noises = _draw_banks()
    calls = _capture(monkeypatch)
    out = _transform(dev, None, noises, aug_seed=8, noise_prob=NOISE_PROB, tr_snr=[0.0, 20.0]).train_transform(clips)
    assert not calls["ir"]
    mix = calls["mix"][0]
    on = mix["index"] >= 0
    x, got = clips.cpu().numpy().astype(np.float64), out.cpu().numpy().astype(np.float64)
    added = got[on] - x[on]
    realised = 20.0 * np.log10(np.sqrt((x[on] ** 2).mean(axis=1)) / np.sqrt((added ** 2).mean(axis=1)))
    worst = float(np.abs(realised - mix["snr"][on].astype(np.float64)).max())
    print(f"augment-draws realised SNR: worst deviation {worst:.2e} dB over {int(on.sum())} clips")
    assert worst < 2e-3
    assert np.array_equal(_bits(out.cpu().numpy()[~on]), _bits(clips.cpu().numpy()[~on]))
