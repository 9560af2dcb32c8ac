"""GPU tests of every route of the dynamic k-NN graph -- knn_graph.hip (exact f32, PIPE and generic), knn_pre.hip (bf16
pre-filter), knn_split.hip (split form for f32 inputs, raw form for bf16 inputs, the exact passes 3a / 3b) -- at the shapes
of tests/_knn_ref.py: all routes equal each other, equal the C oracle bit for bit, and pass the two float64 rules stated
there.  tests/test_knn_cpu.py shows on the CPU that the oracle meets the rules, what share of the queries the equality
rule covers and which exact pass every planted query reaches.  Every input is a view into a larger buffer with a guard
of a fixed finite value on both sides; the direct C-entry calls guard the index output and the workspace as well.  Every
comparison prints its worst error-to-bar ratio and the uncertified share.  `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

import _knn_ref as kr

pytestmark = pytest.mark.gpu

GUARD, GUARD_VALUE = 1024, 24576.0             # elements on each side of an input / behind an index output (bf16 holds it)
GUARD_BYTES, GUARD_BYTE = 4096, 0xA5           # behind a workspace
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
ALL_CASES = kr.CASES + kr.PRE_CASES


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


class Guarded:
    """A (B, C, N) array on the device in `layout`, as a contiguous view into a larger buffer: GUARD elements of
    GUARD_VALUE in front (+ `offset` elements: the view's misalignment) and behind.  intact() after the kernels ran."""

    def __init__(self, a, dtype, layout, dev, offset=0):
        t = torch.tensor(np.asarray(a), device=dev).to(TDT[dtype])      # a copy: the cached inputs stay read-only
        if layout == "cbn":
            t = t.permute(1, 0, 2).contiguous()
        self.front = GUARD + offset
        self.buf = torch.full((self.front + t.numel() + GUARD,), GUARD_VALUE, dtype=t.dtype, device=dev)
        self.x = self.buf[self.front:self.front + t.numel()].view(t.shape)
        self.x.copy_(t)
        self.want = t
        assert self.x.is_contiguous() and self.buf.data_ptr() % 16 == 0
        assert (self.x.data_ptr() % 16 == 0) == (offset * t.element_size() % 16 == 0)

    def intact(self):
        torch.cuda.synchronize()
        n = self.want.numel()
        assert bool((self.buf[:self.front] == GUARD_VALUE).all()) and bool((self.buf[self.front + n:] == GUARD_VALUE).all()), \
            "a kernel wrote around its input"
        assert torch.equal(self.x, self.want), "a kernel wrote into its input"


def _strides(layout, B, C, N):
    return (C * N, N) if layout == "bcn" else (N, B * N)


def _abi(dev, entry, g, layout, B, C, N, k, idx32, ws_query, normalize=None):
    """grafp_knn_graph_split / grafp_knn_graph_pre on a guarded input: the index output pre-filled with an out-of-range
    value and followed by GUARD elements of another, the workspace 0xFF bytes followed by GUARD_BYTES of 0xA5.
    Returns (rc, idx (B, N, k) on the device, uncertified count or None)."""
    from grafp_amd import ops
    lib, p = ops.lib, ops._p
    dt = ops._DT[g.x.dtype]
    sb, sc = _strides(layout, B, C, N)
    n = B * N * k
    out = torch.full((n + GUARD,), N + 7, dtype=torch.int32 if idx32 else torch.int64, device=dev)
    out[n:] = -5
    nbytes = ws_query(dt)
    ws = torch.full((nbytes + GUARD_BYTES,), 0xFF, dtype=torch.uint8, device=dev)
    ws[nbytes:] = GUARD_BYTE
    assert ws.data_ptr() % 16 == 0 and nbytes > 0
    if entry == "split":
        unc = torch.full((), -1, dtype=torch.int32, device=dev)
        rc = lib.grafp_knn_graph_split(p(g.x), dt, sb, sc, B, C, N, k, p(out), int(idx32), p(ws), nbytes, p(unc), ops._stream())
    else:
        unc = None
        rc = lib.grafp_knn_graph_pre(p(g.x), dt, sb, sc, B, C, N, k, int(normalize), p(out), int(idx32), p(ws), nbytes,
                                     ops._stream())
    torch.cuda.synchronize()
    assert bool((out[n:] == -5).all()), "a kernel wrote past the index output"
    assert bool((ws[nbytes:] == GUARD_BYTE).all()), "a kernel wrote past the reported workspace"
    return rc, out[:n].view(B, N, k), unc


def _split_abi(dev, g, layout, B, C, N, k, idx32):
    from grafp_amd import ops
    rc, idx, unc = _abi(dev, "split", g, layout, B, C, N, k, idx32,
                        lambda dt: ops.lib.grafp_knn_split_workspace_for(dt, B, C, N))
    assert rc == 0, ops.lib.grafp_last_error()
    return idx, int(unc)


def _pre_abi(dev, g, layout, B, C, N, k, idx32, normalize=True):
    from grafp_amd import ops
    rc, idx, _ = _abi(dev, "pre", g, layout, B, C, N, k, idx32, lambda dt: ops.lib.grafp_knn_pre_workspace(B, C, N), normalize)
    assert rc == 0, ops.lib.grafp_last_error()
    return idx


def _same(results, want, what):
    """Every route's indices equal the oracle's (hence each other), bit for bit."""
    for name, idx in results.items():
        got = idx.cpu().numpy().astype(np.int64)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{what} {name}: {len(bad)} of {got.size} indices differ from the oracle; first {bad[:4].tolist()}"


# ================================================================================================ the case table
@pytest.mark.parametrize("dtype", kr.DTYPES)
@pytest.mark.parametrize("c", ALL_CASES, ids=kr.case_id)
def test_every_route_vs_oracle_and_float64(dev, c, dtype):
    """k = 1, 3, 4 through the default route, ops.knn_graph_split, the split C entry (guarded output and workspace),
    prefilter=False (knn_graph.hip) and, where C % 64 == 0, prefilter=True and the pre-filter's C entry; at k = 3 also the
    (C, B, N) layout and int32 indices.  The uncertified count is at least the number of planted queries that float64
    shows to be uncertified whatever the rounding; no upper bound is fixed (the key truncation exceeds the band from 11
    index bits on)."""
    from grafp_amd import ops
    from oracle import native
    B, C, N = c.B, c.C, c.N
    x, ref = kr.inputs(c, dtype), kr.cached_ref(c, dtype)
    g = Guarded(x, dtype, "bcn", dev)
    gc = Guarded(x, dtype, "cbn", dev)
    assert ops.lib.grafp_knn_split_preferred_for(ops._DT[TDT[dtype]], C, N, 3) == (c.pref_f32 if dtype == "f32" else c.pref_bf16)
    for k in kr.K_GPU:
        what = f"{kr.case_id(c)} {dtype} k={k}"
        want = native.knn_graph(x, k)
        i32 = k != 3
        res = {"default": ops.knn_graph(g.x, k), "exact-f32": ops.knn_graph(g.x, k, prefilter=False)}
        res["split"], unc_ops = ops.knn_graph_split(g.x, k, return_uncertified=True)
        res["split entry"], unc = _split_abi(dev, g, "bcn", B, C, N, k, i32)
        if c.pre:
            res["pre-filter"] = ops.knn_graph(g.x, k, prefilter=True)
            res["pre-filter entry"] = _pre_abi(dev, g, "bcn", B, C, N, k, i32)
        if k == 3:
            res["default cbn"] = ops.knn_graph(gc.x, k, layout="cbn")
            res["default cbn int32"] = ops.knn_graph(gc.x, k, layout="cbn", index_dtype=torch.int32)
            res["exact-f32 cbn"] = ops.knn_graph(gc.x, k, layout="cbn", prefilter=False)
            res["split entry cbn"], unc_c = _split_abi(dev, gc, "cbn", B, C, N, k, True)
            assert unc_c == unc
            if c.pre:
                res["pre-filter entry cbn"] = _pre_abi(dev, gc, "cbn", B, C, N, k, False)
        assert res["split entry"].dtype == (torch.int32 if i32 else torch.int64) and res["default"].dtype == torch.int64
        _same(res, want, what)
        kr.check(res["default"].cpu().numpy(), ref, C, what)
        planted = kr.sure_uncertified_planted(c, dtype, k)
        print(f"knn {what}: uncertified {unc} of {B * N} queries ({100.0 * unc / (B * N):.2f} %), planted and surely "
              f"uncertified {planted}")
        assert int(unc_ops) == unc and planted <= unc <= B * N
    g.intact()
    gc.intact()


@pytest.mark.parametrize("dtype", kr.DTYPES)
def test_1024_channels_take_the_exact_route_and_agree(dev, dtype):
    """C = 1024 is past the split form's error budget: the default route is knn_graph.hip, the split wrapper and the split
    C entry refuse (the entry before any launch: output and workspace untouched), the pre-filter still runs."""
    from grafp_amd import ops
    from oracle import native
    c = kr.UNSUPPORTED
    B, C, N = c.B, c.C, c.N
    x, ref = kr.inputs(c, dtype), kr.cached_ref(c, dtype)
    g = Guarded(x, dtype, "bcn", dev)
    for k in kr.K_GPU:
        res = {"default": ops.knn_graph(g.x, k), "exact-f32": ops.knn_graph(g.x, k, prefilter=False),
               "pre-filter": ops.knn_graph(g.x, k, prefilter=True), "pre-filter entry": _pre_abi(dev, g, "bcn", B, C, N, k, k == 1)}
        _same(res, native.knn_graph(x, k), f"{kr.case_id(c)} {dtype} k={k}")
        kr.check(res["default"].cpu().numpy(), ref, C, f"{kr.case_id(c)} {dtype} k={k}")
    with pytest.raises(ValueError, match="unsupported shape"):
        ops.knn_graph_split(g.x, 3)
    rc, idx, unc = _abi(dev, "split", g, "bcn", B, C, N, 3, False, lambda dt: 1 << 20)
    assert rc == -1 and b"unsupported shape" in ops.lib.grafp_last_error()               # GRAFP_ERR_ARG
    assert bool((idx == N + 7).all()) and int(unc) == -1
    g.intact()


# ================================================================================================ all-HEAVY clips
@pytest.mark.parametrize("dtype", kr.DTYPES)
def test_all_heavy_clips_of_640_nodes(dev, dtype):
    """(64, 640): every node identical, and one-hot features (exact ties at distance 2).  Every query takes pass 3b, 40
    groups of 16 over two column ranges, the second of 128 columns: the lowest indices win, exactly."""
    from grafp_amd import ops
    from oracle import native
    x = kr.heavy_clips()
    ref = kr.make_ref(x)
    g = Guarded(x, dtype, "bcn", dev)
    for k in kr.K_GPU:
        idx, unc = _split_abi(dev, g, "bcn", 2, 64, 640, k, k == 1)
        assert unc == 2 * 640
        _same({"split entry": idx, "default": ops.knn_graph(g.x, k), "exact-f32": ops.knn_graph(g.x, k, prefilter=False)},
              native.knn_graph(x, k), f"all-HEAVY {dtype} k={k}")
        kr.check_exact(idx.cpu().numpy(), ref, f"all-HEAVY {dtype} k={k}")
    g.intact()


# ================================================================================================ pass 3b's last range
@pytest.mark.parametrize("dtype", kr.DTYPES)
@pytest.mark.parametrize("C,N,B", [(64, 640, 3), (64, 1152, 2)])
def test_heavy_pass_stops_at_the_end_of_the_clip(dev, C, N, B, dtype):
    """Pass 3b walks the candidates in ranges of 512 columns; the last range of a clip with N % 512 = 128 must end after
    128.  In the (C, B, N) layout the 384 columns behind it are columns 0 .. 383 of the NEXT clip: an exact copy of a
    HEAVY query of clip 0 sits there (clip 1, column 100), where a range of 512 would find it at distance 0 and return
    the index N + 100.  Every index is below N and equals the oracle's.  The last clip holds a cluster INSIDE the short
    range (columns N - 26 .. N - 2: a pass that dropped the range would lose every neighbour of theirs) and one across
    the first range boundary (columns 500 .. 524)."""
    from grafp_amd import ops
    from oracle import native
    x = kr.hash_normalish(f"knn64:ragged.{C}.{N}", (B, C, N)).astype(np.float32)
    clusters = ((0, kr.CLUSTER_COLS), (B - 1, np.arange(N - 26, N - 1)), (B - 1, np.arange(500, 525)))
    for i, (b, cols) in enumerate(clusters):
        noise = kr.hash_normalish(f"knn64:ragged.cluster{i}.{C}.{N}", (C, len(cols)))
        x[b][:, cols] = x[b][:, cols[:1]] + np.float32(1e-3) * noise
    member = int(kr.CLUSTER_COLS[3])
    assert 100 < 512 - N % 512 and N % 512 == 128
    x[1, :, 100] = x[0, :, member]
    if dtype == "bf16":
        x = kr.to_bf16(x)
    ref = kr.make_ref(x)
    planted = {}
    for k in kr.K_GPU:                                              # the cluster members are HEAVY whatever the rounding
        unc_sure, _, heavy = kr.sure_tiers(ref, k, kr.band(C, dtype))
        assert heavy[0, member] and all(heavy[b, cols].sum() >= (10 if k == 1 else len(cols)) for b, cols in clusters[1:])
        planted[k] = sum(int(unc_sure[b, cols].sum()) for b, cols in clusters)
    assert (ref.order[B - 1, N - 26:N - 1, 1:4] >= N - 128).all()  # neighbours out of the short range only
    across = ref.order[B - 1, 500:525, :4]
    assert (across < 512).any() and (across >= 512).any()
    g = Guarded(x, dtype, "cbn", dev)
    for k in kr.K_GPU:
        what = f"ragged {C}-{N} {dtype} k={k}"
        idx, unc = _split_abi(dev, g, "cbn", B, C, N, k, k == 1)
        default = ops.knn_graph(g.x, k, layout="cbn")
        assert int(idx.max()) < N and int(default.max()) < N and int(idx.min()) >= 0, what
        _same({"split entry": idx, "default": default}, native.knn_graph(x, k), what)
        kr.check(idx.cpu().numpy(), ref, C, what)
        print(f"knn {what}: uncertified {unc} of {B * N} queries, cluster members surely uncertified {planted[k]}")
        assert planted[k] >= 40 and unc >= planted[k]
    g.intact()


# ================================================================================================ misaligned views
@pytest.mark.parametrize("layout", ["bcn", "cbn"])
@pytest.mark.parametrize("dtype", kr.DTYPES)
def test_view_at_storage_offset_1_takes_the_exact_route(dev, dtype, layout):
    """A contiguous view whose first element is not 16-byte aligned: the split entry refuses it (its loads are 16 bytes
    wide), so the default route must not choose it -- it returns the oracle's graph through knn_graph.hip."""
    from grafp_amd import ops
    from oracle import native
    c = kr.CASES[2]
    B, C, N = c.B, c.C, c.N
    x, ref = kr.inputs(c, dtype), kr.cached_ref(c, dtype)
    g = Guarded(x, dtype, layout, dev, offset=1)
    assert g.x.data_ptr() % 16 != 0 and g.x.storage_offset() == GUARD + 1
    assert ops.lib.grafp_knn_split_preferred_for(ops._DT[TDT[dtype]], C, N, 3) == 1
    for k, dt_i in ((3, torch.int64), (4, torch.int32)):
        got = ops.knn_graph(g.x, k, layout=layout, index_dtype=dt_i)
        assert got.dtype == dt_i
        _same({"default": got, "pre-filter": ops.knn_graph(g.x, k, layout=layout, prefilter=True)}, native.knn_graph(x, k),
              f"offset-1 view {dtype} {layout} k={k}")
        kr.check(got.cpu().numpy(), ref, C, f"offset-1 view {dtype} {layout} k={k}")
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.knn_graph_split(g.x, 3, layout=layout)
    g.intact()


# ================================================================================================ integer features
@pytest.mark.parametrize("C,N,B,form", [(64, 640, 3, "PIPE up to k = 4, generic from k = 5"), (96, 384, 3, "generic: C % 64 != 0"),
                                         (40, 300, 2, "generic, ragged tiles: N % 128 = 44")])
def test_unnormalised_integer_features_equal_the_float64_argsort(dev, C, N, B, form):
    """normalize=False on integers in [-3, 3]: exact in f32 and f64, many exact ties -- idx is the float64 stable argsort
    for EVERY query, k = 1 .. 8, through knn_graph.hip (and the pre-filter where it applies, whose bounds are loose here:
    the exact fallback everywhere)."""
    from grafp_amd import ops
    x = kr.int_inputs(C, N, B)
    ref = kr.make_ref(x, normalize=False)
    g = Guarded(x, "f32", "bcn", dev)
    gb = Guarded(x, "bf16", "cbn", dev)                             # small integers: bf16 holds them
    for k in range(1, 9):
        kr.check_exact(ops.knn_graph(g.x, k, normalize=False).cpu().numpy(), ref, f"int {C}-{N} k={k} ({form})")
        kr.check_exact(ops.knn_graph(gb.x, k, normalize=False, layout="cbn", index_dtype=torch.int32).cpu().numpy(), ref,
                       f"int {C}-{N} k={k} bf16 cbn")
        if k <= 4 and ops.lib.grafp_knn_pre_supported(C, N, k):
            kr.check_exact(ops.knn_graph(g.x, k, normalize=False, prefilter=True).cpu().numpy(), ref, f"int {C}-{N} k={k} pre-filter")
            kr.check_exact(_pre_abi(dev, g, "bcn", B, C, N, k, False, normalize=False).cpu().numpy(), ref,
                           f"int {C}-{N} k={k} pre-filter entry")
    g.intact()
    gb.intact()


# ================================================================================================ the wide norm kernels
@pytest.mark.parametrize("B,ve", [(8192, 4), (16384, 8)])
def test_raw_form_norm_kernels_of_4_and_8_nodes_per_thread(dev, B, ve):
    """bf16 inputs of 2^20 / 2^21 nodes make the raw form's pass 1 take 4 / 8 nodes per thread (8- / 16-byte loads).  At
    C = 32, N = 128: every clip equals the exact-f32 route, seven clips equal the C oracle on the widened values."""
    from grafp_amd import ops
    from oracle import native
    C, N, k = 32, 128, 3
    assert B * N == (1 << 20) * (ve // 4)
    gen = torch.Generator(device=dev).manual_seed(B)
    buf = torch.full((GUARD + B * C * N + GUARD,), GUARD_VALUE, dtype=torch.bfloat16, device=dev)
    x = buf[GUARD:GUARD + B * C * N].view(B, C, N)
    x.copy_(torch.randn(B, C, N, device=dev, generator=gen))
    keep = x.clone()
    idx, unc = ops.knn_graph_split(x, k, return_uncertified=True)
    assert torch.equal(idx, ops.knn_graph(x, k, prefilter=False))
    assert torch.equal(idx, ops.knn_graph(x, k))
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    print(f"knn raw norms x{ve}: uncertified {int(unc)} of {B * N} queries ({100.0 * int(unc) / (B * N):.3f} %)")
    for b in (0, B - 1) + tuple(range(B // 6, B - 1, B // 6))[:5]:
        assert np.array_equal(idx[b].cpu().numpy(), native.knn_graph(x[b:b + 1].float().cpu().numpy(), k)[0]), b
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == GUARD_VALUE).all()) and bool((buf[GUARD + B * C * N:] == GUARD_VALUE).all())
    assert torch.equal(x, keep)
