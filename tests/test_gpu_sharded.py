"""The sharded fingerprint library on the MI355X: grafp_merge_track_lists_f32 against its numpy restatement
(tests/_shard_ref.py) at the limits of the merge, and ShardedFingerprintLibrary (grafp_amd/sharded.py) against the
one-card FingerprintLibrary over the same tracks -- `==` on the returned Python structures, floats included -- for
identify, identify_windows, timeline, match, their tempo forms, a thinned library, the search, the constructors, the files
and StreamMonitor.  All shards sit on the test device; two devices are used where the box has them."""
import numpy as np
import pytest
import torch

from _retrieval_case import synth_tracks
from _shard_ref import merge_ref, random_lists
from grafp_amd import ops
from grafp_amd.library import FingerprintLibrary
from grafp_amd.monitor import StreamMonitor
from grafp_amd.sharded import ShardedFingerprintLibrary, split_tracks
from grafp_amd.train import build_model
from grafp_amd.util import load_config

pytestmark = pytest.mark.gpu
SEG_HOP = 3 * 512                     # samples between segment starts at the default settings (0.096 s)
SHARDS = [1, 2, 3, 8, 11]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---- the kernel against the restatement -----------------------------------------------------------------------------
def _merge(dev, track, score, payload, base, pad):
    t = lambda a: torch.from_numpy(a).to(dev)
    out = ops.merge_track_lists(t(track), t(score), t(payload), base, pad)
    return [o.cpu().numpy() for o in out]


def _same(got, want, what=""):
    for g, x, name in zip(got, want, ("track", "score", "payload")):
        assert g.dtype == x.dtype and g.shape == x.shape and np.array_equal(g, x), (what, name, np.argwhere(g != x)[:5])


@pytest.mark.parametrize("S,n_items,top,P,keep", [(1, 1, 1, 0, 1.0), (2, 7, 5, 2, 0.5), (3, 41, 5, 3, 1.0),
                                                  (8, 33, 8, 5, 0.8), (64, 3, 64, 4, 0.9), (64, 2, 1, 2, 0.7)])
def test_kernel_matches_restatement_with_ties(dev, S, n_items, top, P, keep):
    """Scores from four values: ties inside and across the shards' lists, decided by the global track."""
    case = random_lists(100 + S + top, S, n_items, top, P, tracks_per_shard=max(9, top + 3), keep=keep)
    track, score = case[0], case[1]
    got = _merge(dev, *case)
    want = merge_ref(*case)
    filled = int((want[0] >= 0).sum())
    ties = int(((want[1][:, 1:] == want[1][:, :-1]) & (want[0][:, 1:] >= 0)).sum())     # equal scores side by side
    print(f"S={S} n_items={n_items} top={top} P={P}: {int((track >= 0).sum())} entries in, {filled} out, "
          f"{ties} ties between neighbours")
    _same(got, want)
    assert filled > 0 and (top == 1 or S * top < 8 or ties > 0)
    if keep < 1.0 and S * top > 4:
        assert (track < 0).any()                                 # padding inside the lists was skipped


def test_all_padding_no_items_the_mark_and_the_identity(dev):
    track, score, payload, base, pad = random_lists(5, 4, 6, 5, 3)
    # every entry padding: every output is its padding, whatever the scores say
    got = _merge(dev, np.full_like(track, -1), score, payload, base, pad)
    assert (got[0] == -1).all() and (got[1] == -np.inf).all()
    assert all((got[2][p] == pad[p]).all() for p in range(3))
    # no items: nothing is launched
    none = _merge(dev, track[:, :0], score[:, :0], payload[:, :, :0], base, pad)
    assert [o.shape for o in none] == [(0, 5), (0, 5), (3, 0, 5)]
    # cross_match's -2 in any entry of an item goes to the item's slot 0
    marked = track.copy()
    marked[2, 1, 3], marked[0, 4, 0] = -2, -2
    got = _merge(dev, marked, score, payload, base, pad)
    _same(got, merge_ref(marked, score, payload, base, pad))
    assert got[0][1].tolist() == [-2, -1, -1, -1, -1] and got[0][4, 0] == -2 and (got[0][[0, 2, 3, 5], 0] >= 0).all()
    # one shard: the identity on the non-padding prefix, padding rewritten as padding
    track, score, payload, base, pad = random_lists(6, 1, 20, 7, 2, keep=0.6)
    got = _merge(dev, track, score, payload, base, pad)
    assert np.array_equal(got[0], track[0]) and np.array_equal(got[1], score[0]) and np.array_equal(got[2], payload[:, 0])
    # `top` cuts the result, and P = 0 carries nothing
    t = lambda a: torch.from_numpy(a).to(dev)
    cut = ops.merge_track_lists(t(track), t(score), None, base, [], top=3)
    assert [tuple(o.shape) for o in cut] == [(20, 3), (20, 3), (0, 20, 3)]
    assert np.array_equal(cut[0].cpu().numpy(), track[0][:, :3])


# ---- the library end to end ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(dev):
    """test_gpu_identify_tempo.py's small recipe: an untrained model, 8 tracks of 84 segment hops; the dense f32 library."""
    cfg = load_config()
    torch.manual_seed(0)
    model = build_model(cfg, device=dev).eval()
    tracks = synth_tracks(8, 84 * SEG_HOP / 16000, 4242, dev)
    names = [f"song{i}" for i in range(8)]
    lib = FingerprintLibrary.build(model, list(tracks), cfg, names=names, precision="f32", max_segments=200)
    return cfg, model, tracks, names, lib


def _calls(tracks):
    """The query calls of the end-to-end comparison, by name: lib -> result."""
    crops = [tracks[i % 8, 3000 * i:3000 * i + 20000 + 4000 * i] for i in range(10)]          # ragged: 1.25 s to 3.5 s
    long_crops = [tracks[i % 8, 3000 * i:3000 * i + 56000] for i in range(10)]
    recordings = [torch.cat([tracks[2], tracks[5]]), tracks[6, 10 * SEG_HOP:10 * SEG_HOP + 5 * 16000]]
    return {
        "identify": lambda lib: lib.identify(crops, top=5),
        "identify_tempo": lambda lib: lib.identify(long_crops, fs=16640, top=5, tempo=0.06),
        "windows": lambda lib: lib.identify_windows(tracks[2]),
        "windows_tempo": lambda lib: lib.identify_windows(tracks[2], fs=16640, tempo=0.06),
        "match": lambda lib: lib.match(recordings),
        "match_tempo": lambda lib: lib.match(recordings, tempo=0.06),
    }


THIN_CALLS = ("identify", "windows")


@pytest.fixture(scope="module")
def want(small):
    """What the one-card libraries (dense, and every second row) return: computed once."""
    cfg, model, tracks, names, lib = small
    calls = _calls(tracks)
    dense = {name: call(lib) for name, call in calls.items()}
    thin_lib = lib.thin(2)
    thin = {name: calls[name](thin_lib) for name in THIN_CALLS}
    assert sum(bool(r) for r in dense["identify"]) >= 8                       # (an untrained model: no accuracy asked)
    assert all("tempo" in r[0] for r in dense["identify_tempo"])
    assert {m["track"] for m in dense["match"][0][:2]} == {2, 5} and dense["match"][1][0]["track"] == 6   # exact rows
    assert dense["match_tempo"][0] and "tempo" in dense["match_tempo"][0][0]
    assert len(dense["windows"]) >= 5 and all(w["matches"] for w in dense["windows"])
    return dense, thin_lib, thin


@pytest.mark.parametrize("S", SHARDS)
def test_sharded_queries_equal_the_one_card_library(small, want, S):
    cfg, model, tracks, names, lib = small
    dense, thin_lib, thin = want
    sh = ShardedFingerprintLibrary.split(lib, S)
    assert len(sh.shards) == S and sh.tb.tolist() == split_tracks(lib.first, S).tolist()
    if S == 11:
        assert sum(part.n_rows == 0 for part in sh.shards) >= 3            # shards without rows launch nothing
    for name, call in _calls(tracks).items():
        got = call(sh)
        assert got == dense[name], (S, name)
        if name.startswith("windows"):
            assert sh.timeline(got) == lib.timeline(dense[name]) and sh.timeline(got), (S, name)
    sh_thin = ShardedFingerprintLibrary.split(thin_lib, S)
    assert sh_thin.row_stride == 2
    for name in THIN_CALLS:
        got = _calls(tracks)[name](sh_thin)
        assert got == thin[name], (S, name, "thin")
        if name == "windows":
            assert sh_thin.timeline(got) == thin_lib.timeline(thin[name])
    # a single query comes back as its list alone, as from the library
    assert sh.identify(tracks[3, :40000]) == lib.identify(tracks[3, :40000])


def _copy(lib):
    return FingerprintLibrary(lib.model, lib.settings, lib.rows().clone(), lib.first.copy(), list(lib.names),
                              precision=lib.precision, device=lib.device)


@pytest.mark.parametrize("S", SHARDS)
def test_merged_search_is_the_one_card_search(small, S):
    cfg, model, tracks, names, lib = small
    q = lib._embed(lib.segments(torch.cat([tracks[1, 5000:60000], tracks[7, :30000]])))
    sh = ShardedFingerprintLibrary.split(lib, S)
    got, ref = sh._search_rows(q, 20), lib._search_rows(q, 20)
    assert got.dtype == ref.dtype and got.shape == ref.shape == (q.shape[0], 20) and torch.equal(got, ref), S
    # more hits asked for than the library has rows: k is the row count, as on one card
    few = ShardedFingerprintLibrary.split(lib.thin(32), S)
    assert few.n_rows < 32 and torch.equal(few._search_rows(q, 32), lib.thin(32)._search_rows(q, 32))


def test_a_shard_with_fewer_rows_than_k_probe(small):
    """A ninth track of one segment: split(., 8) leaves it alone in the last shard, whose search returns one hit per row
    and is padded to k_probe."""
    cfg, model, tracks, names, lib = small
    one = tracks[4, 7000:7000 + 31 * 512 + 256]                               # 32 frames: exactly one segment
    lib9 = _copy(lib).add([one], names=["tiny"])
    assert lib9.n_tracks == 9 and lib9.n_rows == lib.n_rows + 1
    sh = ShardedFingerprintLibrary.split(lib9, 8)
    assert sh.shards[-1].n_rows == 1 and sh.shards[-1].names == ["tiny"]
    q = lib._embed(lib.segments(torch.cat([one, tracks[0, :40000]])))
    assert torch.equal(sh._search_rows(q, 20), lib9._search_rows(q, 20))
    crops = [one, tracks[4, 5000:45000], tracks[0, :30000]]
    got, ref = sh.identify(crops, min_overlap=1), lib9.identify(crops, min_overlap=1)
    assert got == ref and ref[0][0]["name"] == "tiny"
    assert sh.match([tracks[4]]) == lib9.match([tracks[4]])


def test_build_add_rebalance_save_and_load(small, want, tmp_path):
    cfg, model, tracks, names, lib = small
    dense = want[0]
    calls = _calls(tracks)
    kw = dict(names=names, precision="f32", max_segments=200)
    built = ShardedFingerprintLibrary.build(model, list(tracks), cfg, n_shards=3, **kw)
    ref = ShardedFingerprintLibrary.split(lib, 3)
    assert built.tb.tolist() == ref.tb.tolist() and built.names == names
    assert all(torch.equal(a.rows(), b.rows()) and np.array_equal(a.first, b.first)
               for a, b in zip(built.shards, ref.shards))
    assert calls["identify"](built) == dense["identify"]
    # shards closed as they fill: the same rows, cut where a shard first holds 150 of them; the last takes the rest
    filled = ShardedFingerprintLibrary.build(model, list(tracks), cfg, n_shards=3, rows_per_shard=150, **kw)
    per = int(lib.first[1])
    assert [part.n_tracks for part in filled.shards] == [-(-150 // per), -(-150 // per), 8 - 2 * -(-150 // per)]
    assert torch.equal(torch.cat([part.rows() for part in filled.shards]), lib.rows())
    assert np.array_equal(filled.first, lib.first) and filled.names == names
    assert calls["match"](filled) == dense["match"]
    # add() appends to the last shard; the results are those of the library that got the same tracks
    more = synth_tracks(2, 60 * SEG_HOP / 16000, 99, lib.device)
    grown = _copy(lib).add(list(more))
    built.add(list(more))
    assert built.names == grown.names and built.names[-2:] == ["track8", "track9"]
    assert np.array_equal(built.first, grown.first) and built.tb.tolist() == ref.tb.tolist()[:3] + [10]
    queries = [more[1, 2 * SEG_HOP:2 * SEG_HOP + 48000], tracks[5, :40000]]      # the first on the segment grid
    ref_id, ref_match = grown.identify(queries), grown.match([more[0]])
    assert ref_id[0][0]["track"] == 9 and ref_match[0][0]["track"] == 8
    assert built.identify(queries) == ref_id and built.match([more[0]]) == ref_match
    # rebalance() is split() of the concatenation
    built.rebalance()
    assert built.tb.tolist() == split_tracks(grown.first, 3).tolist() and np.array_equal(built.first, grown.first)
    assert torch.equal(torch.cat([part.rows() for part in built.shards]), grown.rows())
    assert built.identify(queries) == ref_id
    # the files
    out = str(tmp_path / "sharded")
    built.save(out)
    back = ShardedFingerprintLibrary.load(out, model)
    assert back.tb.tolist() == built.tb.tolist() and back.names == built.names and back.device == lib.device
    assert back.identify(queries) == ref_id and back.match([more[0]]) == ref_match
    assert back.nbytes == sum(part.nbytes for part in back.shards) >= 772 * back.n_rows


def test_stream_monitor_on_a_sharded_library(small):
    cfg, model, tracks, names, lib = small
    sh = ShardedFingerprintLibrary.split(lib, 3)
    streams = [torch.cat([tracks[1, 5 * SEG_HOP:68 * SEG_HOP], tracks[4, 12 * SEG_HOP:74 * SEG_HOP]]),
               tracks[6, 3000:3000 + 7 * 16000]]
    a, b = StreamMonitor(lib, 2, max_chunk_s=1.0), StreamMonitor(sh, 2, max_chunk_s=1.0)
    seen = 0
    for s in range(12):
        chunks = [x[s * 16000:(s + 1) * 16000] if s * 16000 < x.numel() else None for x in streams]
        got, ref = b.push(chunks), a.push(chunks)
        assert got == ref, s
        seen += sum(len(w) for w in ref)
    got, ref = b.end([0, 1]), a.end([0, 1])
    assert got == ref and seen + sum(len(w) for w in ref) >= 12
    assert [b.timeline(ch) for ch in (0, 1)] == [a.timeline(ch) for ch in (0, 1)]
    assert {s["track"] for s in a.timeline(0)} >= {1, 4}


def test_shards_on_two_devices(small, want):
    """Differs from the one-device path only by torch's .to(device) copies; skipped on a box with one GPU."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    cfg, model, tracks, names, lib = small
    sh = ShardedFingerprintLibrary.split(lib, 4, devices=["cuda:0", "cuda:1", "cuda:0", "cuda:1"])
    assert [part.device.index for part in sh.shards] == [0, 1, 0, 1]
    calls = _calls(tracks)
    assert calls["identify"](sh) == want[0]["identify"] and calls["match"](sh) == want[0]["match"]
