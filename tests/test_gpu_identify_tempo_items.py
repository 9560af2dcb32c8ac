"""Identification over a ratio window per item, on the MI355X (csrc/identify_tempo_items.hip, ops.identify_tempo_items):
row i of every output is row 0 of the tempo identification of item i alone over ratio_num[lo_i : lo_i + cnt_i] -- against
the numpy restatement applied per item (tests/_identify_tempo_ref.py, bit-exact on dyadic inputs), against
ops.identify_tempo where every window is the whole grid, on both query-row plans and at the largest item."""
import numpy as np
import pytest
import torch

from _identify_tempo_ref import tempo_case, tempo_ref
from grafp_amd import ops
from test_gpu_identify_tempo import _limit_case

pytestmark = pytest.mark.gpu
NAMES = ("track", "offset", "score", "votes", "ratio")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _run(dev, case, ratios, lo, cnt, top, min_overlap=None, max_len=None):
    t = lambda a: torch.from_numpy(a).to(dev)
    out = ops.identify_tempo_items(*(t(a) for a in case), ratios, lo, cnt, top=top, min_overlap=min_overlap,
                                   max_len=max_len)
    return [o.cpu().numpy() for o in out]


def _whole(dev, case, ratios, top, min_overlap=None, max_len=None):
    t = lambda a: torch.from_numpy(a).to(dev)
    out = ops.identify_tempo(*(t(a) for a in case), ratios, top=top, min_overlap=min_overlap, max_len=max_len)
    return [o.cpu().numpy() for o in out]


def _per_item_ref(case, ratios, lo, cnt, top, min_overlap=None):
    """tempo_ref of every item alone over its own sub-list of ratios, row 0 of each, stacked."""
    rows, first, q, ids, item_row, item_len = case
    per = [tempo_ref(rows, first, q, ids, item_row[i:i + 1], item_len[i:i + 1], ratios[lo[i]:lo[i] + cnt[i]], top=top,
                     min_overlap=min_overlap) for i in range(len(item_row))]
    return [np.concatenate([p[j] for p in per]) for j in range(5)]


def _same(got, want, what=""):
    for g, x, name in zip(got, want, NAMES):
        assert g.dtype == x.dtype and np.array_equal(g, x), (what, name, np.argwhere(g != x)[:5])


@pytest.mark.parametrize("min_overlap", [None, 1, 3])
def test_every_row_is_the_restatement_of_the_item_alone_over_its_window(dev, min_overlap):
    ratios = list(range(240, 273, 4))
    R, n_items = len(ratios), 40
    case = tempo_case(91 + (min_overlap or 0), ratios, n_items, 40, 6)
    cnt = np.array([(1, 3, 9)[i % 3] for i in range(n_items)])
    lo = np.array([(0, (R - c) // 2, R - c)[(i // 3) % 3] for i, c in enumerate(cnt)])
    assert {(int(c), int(a)) for c, a in zip(cnt, lo)} >= {(1, 0), (1, 4), (1, 8), (3, 0), (3, 3), (3, 6), (9, 0)}
    got = _run(dev, case, ratios, lo, cnt, top=8, min_overlap=min_overlap)
    want = _per_item_ref(case, ratios, lo, cnt, top=8, min_overlap=min_overlap)
    found = int((got[0][:, 0] >= 0).sum())
    used = sorted(set(got[4][got[0] >= 0].tolist()))
    print(f"min_overlap={min_overlap}: {found} of {n_items} items find something, winning ratios {used}")
    _same(got, want)
    assert found > n_items // 2 and len(used) > 1
    # every reported ratio lies inside the item's own window
    for i in range(n_items):
        assert set(got[4][i][got[0][i] >= 0].tolist()) <= set(ratios[lo[i]:lo[i] + cnt[i]]), i
    # the same launch with max_len given (asynchronous path), as an upper bound too
    for max_len in (int(case[5].max()), int(case[5].max()) + 9):
        _same(_run(dev, case, ratios, lo, cnt, top=8, min_overlap=min_overlap, max_len=max_len), got, max_len)


@pytest.mark.parametrize("which", ["one", "three", "sixty-four"])
def test_whole_grid_windows_are_identify_tempo_bit_for_bit(dev, which):
    ratios, n_items, max_ql, top = {"one": ([256], 64, 40, 8), "three": ([243, 256, 269], 64, 40, 8),
                                    "sixty-four": (list(range(225, 289)), 10, 12, 64)}[which]
    case = tempo_case(5 + 10 * len(ratios), ratios, n_items, max_ql, 6)
    lo, cnt = np.zeros(n_items, np.int64), np.full(n_items, len(ratios), np.int64)
    got = _run(dev, case, ratios, lo, cnt, top=top, min_overlap=1)
    want = _whole(dev, case, ratios, top=top, min_overlap=1)
    for g, x, name in zip(got, want, NAMES):
        assert g.dtype == x.dtype and np.array_equal(g.view(np.int32), x.view(np.int32)), name
    assert (got[0][:, 0] >= 0).sum() > n_items // 2
    assert len(ratios) * top <= 4096 and (which != "sixty-four" or len(ratios) * top == 4096)


def test_both_plans_at_the_lds_switch(dev):
    """max_len 191 keeps the query rows in LDS, 192 reads them from global memory (test_gpu_identify_tempo.py states the
    sizes): the same items give the same bits, with windows of one ratio and of three."""
    ratios = [250, 256, 262]
    case = _limit_case([191, 0, 17], 21, 9, ratios)
    for lo, cnt in (([0, 1, 2], [1, 1, 1]), ([0, 0, 0], [3, 3, 3])):
        want = _per_item_ref(case, ratios, lo, cnt, top=8, min_overlap=2)
        for max_len in (191, 192, None):
            _same(_run(dev, case, ratios, lo, cnt, top=8, min_overlap=2, max_len=max_len), want, (cnt, max_len))
        assert want[0][1, 0] == -1 and want[4][1, 0] == 0          # the item of length 0 finds nothing
        assert want[0][0, 0] >= 0 and want[0][2, 0] >= 0


def test_query_rows_from_global_memory_at_the_largest_item(dev):
    """ql = 256 with k = 32 (8192 keys) next to two smaller items, windows of one and of two ratios."""
    ratios = [230, 282]
    case = _limit_case([256, 5, 90], 32, 7, ratios)
    lo, cnt = [1, 0, 0], [1, 2, 1]
    got = _run(dev, case, ratios, lo, cnt, top=16, min_overlap=1)
    _same(got, _per_item_ref(case, ratios, lo, cnt, top=16, min_overlap=1))
    assert (got[0][:, 0] >= 0).all()
    assert set(got[4][0][got[0][0] >= 0].tolist()) == {282} and set(got[4][2][got[0][2] >= 0].tolist()) == {230}


def test_the_empty_launch(dev):
    ratios = list(range(240, 273, 4))
    rows, first, q, ids, item_row, item_len = tempo_case(3, ratios, 4, 8, 6)
    none = (rows, first, q, ids, item_row[:0], item_len[:0])
    for max_len in (None, 8):
        out = _run(dev, none, ratios, [], [], top=7, max_len=max_len)
        assert [o.shape for o in out] == [(0, 7)] * 5
        assert [o.dtype for o in out] == [np.int32, np.int32, np.float32, np.int32, np.int32]
