"""The kernels of csrc/ivfpq.hip against float64 at their tile and list edges (tests/_ivfpq_ref.py has the inputs, the
references, the case tables and the derivation of the two bars; tests/test_ivfpq_cpu.py pins all of that on the CPU).

On the exact inputs every comparison is np.array_equal with the float64 definition: assignments and codes
(pq_assign_kernel: remainder tiles, ties across tiles, every DCAP with d below it, code 255), one Lloyd step
(kmeans_*_kernel: n around the 1024-row chunk, repeated seeds, the tiled assignment inside the loop, sub-spaces of
residuals), the probed lists (ivfpq_probe_kernel: 1 ... 300 lists, ties by list id, a NaN query), the fused search and the
dense scan (ivfpq_search_kernel / ivfpq_adc_kernel: lists of 0 / 1 / 255 / 256 / 257 / 513 rows, equal estimates in two
lists, a query that finds nothing, M = 8 ... 128).  On random unit rows: the assignment certificate and the Lloyd-step
identity, and the bits of oracle/csrc/ivfpq.c."""
import ctypes

import numpy as np
import pytest
import torch

import _ivfpq_ref as ir
from grafp_amd import ivfpq
from grafp_amd._lib import check, lib
from grafp_amd.ivfpq import IVFPQIndex
from oracle import native

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
ERR_ARG, ERR_WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _p(t):
    return vp(t.data_ptr()) if t is not None else None


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def _last_error():
    return lib.grafp_last_error().decode("utf-8", "replace")


# ---- 1. pq_assign, exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ir.ASSIGN_CASES, ids=lambda c: c.name)
def test_pq_assign_is_the_float64_argmin(dev, case):
    c = ir.assign_case(case.name)
    ir.check_exact(c)
    want = ir.ref_assign(c["x"], c["G"], c["cent"], c["base"], c["base_idx"])
    x, cent, base, bi = (_t(c[key], dev) for key in ("x", "cent", "base", "base_idx"))
    got = ivfpq.pq_assign(x, case.G, cent, base, bi)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    if case.k <= 256:
        codes = ivfpq.pq_assign(x, case.G, cent, base, bi, as_codes=True)
        assert codes.dtype == torch.uint8 and np.array_equal(codes.cpu().numpy(), want.astype(np.uint8))
        assert torch.equal(codes.int(), got)
    if case.k == 256:
        assert (got == 255).any(dim=0).all()                                  # the last code, in every sub-space
    # one row (one live thread of the block) and none
    one = ivfpq.pq_assign(x[:1].contiguous(), case.G, cent, base, None if bi is None else bi[:1].contiguous())
    assert np.array_equal(one.cpu().numpy(), want[:1])
    for as_codes, dtype in ((False, torch.int32), (True, torch.uint8)):
        none = ivfpq.pq_assign(x[:0], case.G, cent, base, None if bi is None else bi[:0], as_codes=as_codes)
        assert none.shape == (0, case.G) and none.dtype == dtype
    out = torch.full((4, case.G), -7, dtype=torch.int32, device=dev)         # the C entry with n = 0: nothing is written
    check(lib.grafp_pq_assign_f32(_p(x), 0, case.D, case.G, _p(base), _p(bi), _p(cent), case.k, _p(out), None, _stream()),
          "pq_assign")
    assert (out == -7).all()


def test_pq_assign_refusals_leave_the_output_alone(dev):
    x = torch.zeros((4, 129), device=dev)
    for D, G, k, as_codes, message in ((128, 1, 257, True, r"pq_assign: byte codes need k <= 256 \(k=257\)"),
                                       (129, 1, 3, False, r"pq_assign: 129 dims per sub-space \(<= 128\)")):
        cent = torch.zeros((G, k, D // G), device=dev)
        with pytest.raises(RuntimeError, match=message):
            ivfpq.pq_assign(x[:, :D].contiguous(), G, cent, as_codes=as_codes)
        out = torch.full((4, G), 93, dtype=torch.uint8 if as_codes else torch.int32, device=dev)
        rc = lib.grafp_pq_assign_f32(_p(x[:, :D].contiguous()), 4, D, G, None, None, _p(cent), k,
                                     None if as_codes else _p(out), _p(out) if as_codes else None, _stream())
        torch.cuda.synchronize()
        assert rc == ERR_ARG and (out == 93).all()


# ---- 2. k-means, exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ir.KMEANS_CASES, ids=lambda c: c.name)
def test_kmeans_is_the_exact_lloyd_step(dev, case):
    c = ir.kmeans_case(case.name)
    ir.check_exact(c)
    x, base, bi = (_t(c[key], dev) for key in ("x", "base", "base_idx"))

    def run(niter):
        return ivfpq.kmeans(x, case.G, case.k, niter=niter, seed=ir.KMEANS_SEED, base=base, base_idx=bi)
    assert np.array_equal(run(0).cpu().numpy(), c["cent0"])                   # the seeds' residuals
    first = run(1)
    assert np.array_equal(first.cpu().numpy(), c["cent1"])                    # exact sums, one f32 division, empty keeps
    assert torch.equal(run(1), first)


def test_kmeans_refuses_a_workspace_one_byte_short(dev):
    n, D, G, k = 300, 32, 4, 16
    x = _t(ir.dyadic("ivfpq:ws.x", (n, D), *ir.ROW_GRID), dev)
    init = _t(ir.init_rows(n, k, 1), dev)
    need = int(lib.grafp_kmeans_workspace(n, D, G, k))
    assert need >= n * G * 4 + G * k * (D // G + 1) * 4        # asg | partial | pcnt of one chunk
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    cent = torch.full((G, k, D // G), 777.0, device=dev)
    rc = lib.grafp_kmeans_f32(_p(x), n, D, G, None, None, _p(init), k, 2, _p(cent), _p(ws), need - 1, _stream())
    torch.cuda.synchronize()
    assert rc == ERR_WORKSPACE and f"kmeans: workspace {need - 1} bytes < required {need}" in _last_error()
    assert (cent == 777.0).all()
    check(lib.grafp_kmeans_f32(_p(x), n, D, G, None, None, _p(init), k, 2, _p(cent), _p(ws), need, _stream()), "kmeans")
    assert np.array_equal(cent.cpu().numpy(), native.kmeans(x.cpu().numpy(), G, k, init.cpu().numpy(), 2))


# ---- 3. k-means, random unit rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,M,nlist,n", ir.RANDOM_CASES)
def test_kmeans_within_both_bars_on_random_rows(dev, d, M, nlist, n):
    """The assignment certificate and the Lloyd-step identity (tests/_ivfpq_ref.py) of iteration RANDOM_NITER of both
    k-means of an index, and the bits of oracle/csrc/ivfpq.c."""
    x = ir.random_rows(d, n)
    xt = _t(x, dev)

    def kmeans(_x, G, k, niter, seed, base, base_idx):
        return ivfpq.kmeans(xt, G, k, niter=niter, seed=seed, base=_t(base, dev), base_idx=_t(base_idx, dev)).cpu().numpy()

    def assign(_x, G, cent, base, base_idx):
        return ivfpq.pq_assign(xt, G, _t(cent, dev), _t(base, dev), _t(base_idx, dev)).cpu().numpy()
    for name, G, k, base, base_idx, seed in ir.random_forms(d, M, nlist, n, kmeans, assign):
        prev = kmeans(x, G, k, ir.RANDOM_NITER - 1, seed, base, base_idx)
        last = kmeans(x, G, k, ir.RANDOM_NITER, seed, base, base_idx)
        asg = assign(x, G, prev, base, base_idx)
        cert = ir.assign_certificate(x, G, prev, asg, base, base_idx)
        ratio, kept, empty = ir.lloyd_identity(last, prev, x, G, asg, base, base_idx)
        print(f"ivfpq bars, kernels ({d}, {M}, {nlist}, {n}) {name}: certificate {cert:.4f}, Lloyd {ratio:.4f} of the bar, "
              f"{empty} empty clusters")
        assert cert <= 1.0 and ratio <= 1.0 and kept
        assert np.array_equal(last, native.kmeans(x, G, k, ir.init_rows(n, k, seed), ir.RANDOM_NITER, base, base_idx))
        assert np.array_equal(asg, native.pq_assign(x, G, prev, base, base_idx))


# ---- 4. probe, exact --------------------------------------------------------------------------------------------------------
def _probe(dev, q, cent, nprobe):
    probe = torch.full((q.shape[0], nprobe), -7, dtype=torch.int32, device=dev)
    check(lib.grafp_ivfpq_probe_f32(_p(q), q.shape[0], q.shape[1], _p(cent), cent.shape[0], nprobe, _p(probe), _stream()),
          "ivfpq_probe")
    return probe


@pytest.mark.parametrize("nlist,nprobe,d", ir.PROBE_CASES)
def test_probe_is_the_lexsort_by_distance_and_list(dev, nlist, nprobe, d):
    c = ir.probe_case(nlist, nprobe, d)
    ir.check_exact(c)
    cent = _t(c["cent"], dev)
    got = _probe(dev, _t(c["q"], dev), cent, nprobe).cpu().numpy()
    assert np.array_equal(got, c["probe"])
    if nprobe == nlist:
        assert (np.sort(got, axis=1) == np.arange(nlist)[None]).all()
    q = c["q"].copy()
    q[ir.PROBE_NAN] = np.nan
    got = _probe(dev, _t(q, dev), cent, nprobe).cpu().numpy()
    row = ir.PROBE_NAN[0]
    assert (got[row] == -1).all() and np.array_equal(np.delete(got, row, 0), np.delete(c["probe"], row, 0))


# ---- 5. fused search and dense scan, exact --------------------------------------------------------------------------------
def _search_index(dev, d, M):
    c = ir.search_case(d, M)
    q = c["q"].copy()
    q[ir.SEARCH_NAN] = np.nan
    index = IVFPQIndex.from_codes({"centroids": _t(c["cent"], dev), "codebooks": _t(c["books"], dev)}, _t(c["a"], dev),
                                  _t(c["codes"], dev), device=dev)
    return c, index, _t(q, dev)


def _dense(index, qt, k, **kw):
    """IVFPQIndex.search's route for k > 32, with _search_dense's rows_per_pass in reach."""
    D = torch.full((qt.shape[0], k), float("inf"), device=qt.device)
    I = torch.full((qt.shape[0], k), -1, dtype=torch.int64, device=qt.device)
    codes, ids, start, counts = index._materialise()
    nprobe = max(1, min(int(index.nprobe), index.nlist))
    probe = _probe(qt.device, qt, index.centroids, nprobe)
    index._search_dense(qt, k, probe, nprobe, codes, ids, start, counts, D, I, _stream(), **kw)
    return D, I


def _same(D, I, Dref, Iref):
    return np.array_equal(I.cpu().numpy(), Iref) and np.array_equal(D.double().cpu().numpy(), Dref)


@pytest.mark.parametrize("d,M", ir.SEARCH_SHAPES)
def test_search_equals_the_float64_definition(dev, d, M):
    """Every (nprobe, k) of the fused route (k <= 32) and the dense route (k > 32): ids and distances of
    oracle.ivfpq.search, the padding where fewer than k candidates exist, where every probed list is empty and for the NaN
    query; the dense route in passes of 7 queries; its first 32 columns are the fused route's."""
    c, index, qt = _search_index(dev, d, M)
    ir.check_exact(c)
    for nprobe in ir.SEARCH_NPROBE:
        index.nprobe = nprobe
        Dref, Iref = ir.search_reference(d, M, nprobe)
        got = {k: index.search(qt, k) for k in ir.SEARCH_K_FUSED + ir.SEARCH_K_DENSE}
        for k, (D, I) in got.items():
            assert D.dtype == torch.float32 and I.dtype == torch.int64 and D.shape == I.shape == (9, k)
            assert _same(D, I, Dref[:, :k], Iref[:, :k]), (nprobe, k)
            assert (I[8] == -1).all() and torch.isinf(D[8]).all() and (D[8] > 0).all()           # the NaN query
            if nprobe == 1:                                                                     # only an empty list
                assert (I[0] == -1).all() and torch.isinf(D[0]).all() and (D[0] > 0).all()
            if nprobe == 4:                                                                     # 6 candidates
                assert (I[0, :6] >= 0).sum() == min(k, 6) and (I[0, 6:] == -1).all() and torch.isinf(D[0, 6:]).all()
        D50, I50 = got[50]
        D7, I7 = _dense(index, qt, 50, rows_per_pass=7)
        assert torch.equal(D7, D50) and torch.equal(I7, I50)
        D1p, I1p = _dense(index, qt, 50)
        assert torch.equal(D1p, D50) and torch.equal(I1p, I50)
        assert torch.equal(D50[:, :32], got[32][0]) and torch.equal(I50[:, :32], got[32][1])


@pytest.mark.parametrize("d,M", [(32, 8), (128, 64)])
def test_scan_leaves_the_slots_of_unprobed_lists(dev, d, M):
    """grafp_ivfpq_scan_f32 with probe slots of -1: their ranges of the pre-filled output stay (+inf, -1), every other
    estimate is the one of the full scan, and the full scan selects oracle.ivfpq.search's lists."""
    c, index, qt = _search_index(dev, d, M)
    qt = qt[:8].contiguous()
    nprobe = 4
    codes, ids, start, counts = index._materialise()
    probe = _probe(dev, qt, index.centroids, nprobe)
    lens = counts[probe.long()]
    ostart = (torch.cumsum(lens, 1) - lens).contiguous()
    stride = int(lens.sum(1).max().item())

    def scan(pb):
        dist = torch.full((8, stride), float("inf"), device=dev)
        pos = torch.full((8, stride), -1, dtype=torch.int32, device=dev)
        check(lib.grafp_ivfpq_scan_f32(_p(qt), 8, d, _p(index.centroids), index.nlist, _p(index.codebooks), M, _p(codes),
                                       _p(start), _p(pb), nprobe, _p(ostart), stride, _p(dist), _p(pos), _stream()), "scan")
        return dist.cpu().numpy(), pos.cpu().numpy()
    dist, pos = scan(probe)
    Dref, Iref = ir.search_reference(d, M, nprobe)
    ids_h = ids.cpu().numpy()
    for r in range(8):
        have = pos[r] >= 0
        assert have.sum() == int(lens[r].sum())
        cand_i, cand_d = ids_h[pos[r][have]], dist[r][have].astype(np.float64)
        sel = np.lexsort((cand_i, cand_d))[:50]
        assert np.array_equal(cand_i[sel], Iref[r, :sel.size]) and np.array_equal(cand_d[sel], Dref[r, :sel.size])
    holes = probe.clone()
    holes[:, 1] = -1
    holes[3, :] = -1
    holes[5, 3] = -1
    dist2, pos2 = scan(holes.contiguous())
    gone = np.zeros((8, stride), bool)
    lens_h, ostart_h, holes_h = lens.cpu().numpy(), ostart.cpu().numpy(), holes.cpu().numpy()
    for r in range(8):
        for s in range(nprobe):
            if holes_h[r, s] < 0:
                gone[r, ostart_h[r, s]:ostart_h[r, s] + lens_h[r, s]] = True
    assert gone.sum() > 256
    assert np.isposinf(dist2[gone]).all() and (pos2[gone] == -1).all()
    assert np.array_equal(dist2[~gone], dist[~gone]) and np.array_equal(pos2[~gone], pos[~gone])


# ---- 6. index paths -------------------------------------------------------------------------------------------------------
def test_add_in_chunks_equals_one_add(dev):
    x = np.array(ir.random_rows(32, 2500))
    whole = IVFPQIndex(32, nlist=5, M=8, niter=2, device=dev, keep_raw=False)
    whole.train(x)
    parts = IVFPQIndex.from_codes(whole.quantiser(), torch.zeros(0, dtype=torch.int32), torch.zeros((0, 8), dtype=torch.uint8),
                                  device=dev)
    whole.add(x[:350])
    parts.add(x[:350], chunk=100)
    assert parts.ntotal == whole.ntotal == 350 and len(parts._codes) == 4
    (a1, c1), (a2, c2) = whole.codes_by_row(), parts.codes_by_row()
    assert torch.equal(a1, a2) and torch.equal(c1, c2)
    whole.nprobe = parts.nprobe = 3
    (D1, I1), (D2, I2) = whole.search(x[:20], 10), parts.search(x[:20], 10)
    assert np.array_equal(I1, I2) and np.array_equal(D1, D2)


def test_training_subsample_is_the_documented_selection(dev):
    """More rows than max_points_per_centroid * max(nlist, 256) = 65 536: train(x) is train(x[sel]) with the seeded
    selection of IVFPQIndex.train, whether x is an array, a host tensor or a device tensor."""
    d, n, cap = 16, 65536 + 1000, 65536
    x = ir.hash_normalish("ivfpq:subsample", (n, d))

    def trained(rows):
        index = IVFPQIndex(d, nlist=4, M=16, niter=2, device=dev)
        index.train(rows)
        return index.centroids, index.codebooks
    sel = torch.sort(torch.randperm(n, generator=torch.Generator().manual_seed(1234 + 1))[:cap]).values.numpy()
    assert sel.shape == (cap,) and len(np.unique(sel)) == cap
    want = trained(x[sel])
    for rows in (x, torch.from_numpy(x), torch.from_numpy(x).to(dev)):
        got = trained(rows)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    other = trained(x[:cap])                                   # (the selection matters: other rows, another quantiser)
    assert not torch.equal(other[0], want[0])


def test_empty_index_and_nprobe_clamps(dev):
    c, index, qt = _search_index(dev, 32, 8)
    bare = IVFPQIndex.from_codes(index.quantiser(), torch.zeros(0, dtype=torch.int32), torch.zeros((0, 8), dtype=torch.uint8),
                                 device=dev, nprobe=4)
    assert bare.is_trained and bare.ntotal == 0
    for k in (5, 40):
        D, I = bare.search(qt, k)
        assert D.shape == I.shape == (9, k) and torch.isinf(D).all() and (D > 0).all() and (I == -1).all()
    for asked, served in ((ir.SEARCH_NLIST + 5, ir.SEARCH_NLIST), (0, 1), (-3, 1)):
        for k in (20, 50):
            index.nprobe = asked
            D, I = index.search(qt, k)
            Dref, Iref = ir.search_reference(32, 8, served)
            assert _same(D, I, Dref[:, :k], Iref[:, :k]), (asked, k)


# ---- 7. what the search kernel does not serve is refused when the index is made ---------------------------------------------
def test_index_refuses_unserved_shapes(dev):
    with pytest.raises(ValueError, match=r"d / M = 3 not in \{1, 2, 4, 8\}"):
        IVFPQIndex(d=24, M=8, device=dev)
    with pytest.raises(ValueError, match=r"M = 151 sub-quantisers need 154624 bytes of LDS"):
        IVFPQIndex(d=151, M=151, device=dev)
    IVFPQIndex(d=150, M=150, device=dev)                       # the largest table the search kernel takes
