"""CPU tests of the half form of a fingerprint library (bf16 rows and their norms only: csrc/identify_half.hip,
csrc/crossmatch_half.hip, ops.search_l2_half / identify_half / cross_match_half / HalfL2Index,
FingerprintLibrary.from_half / halve / build(index="half")): the rounding restatement of tests/_half_ref.py, the tables
and the files on device="cpu", every refusal, the routing of the hooks and the shipped assembly.  No GPU call is made."""
import json
import os
import re

import numpy as np
import pytest
import torch

from _common import shipped_asm
from _half_ref import bf16_bits, bf16_values, round_bf16
from grafp_amd import library, ops
from grafp_amd.sharded import ShardedFingerprintLibrary
from grafp_amd.util import load_config

FIRST, TRACK_NAMES = [0, 0, 7, 8, 14], ["a", "b", "c", "d"]


def _tiny_model():
    from grafp_amd.train import build_model
    torch.manual_seed(0)
    return build_model(load_config())


def _f32_rows(n=14, seed=13):
    return np.random.RandomState(seed).randn(n, 128).astype(np.float32)


def _half_lib(model, rows=None):
    bits = bf16_bits(_f32_rows() if rows is None else rows)
    return library.FingerprintLibrary.from_half(model, load_config(), bits, FIRST, TRACK_NAMES, precision="f32",
                                                device="cpu")


def _flat_lib(model):
    return library.FingerprintLibrary(model, load_config(), torch.from_numpy(_f32_rows()), FIRST, TRACK_NAMES,
                                      precision="f32", device="cpu")


def _thin_lib(model):
    return library.FingerprintLibrary(model, load_config(), torch.from_numpy(_f32_rows()), FIRST, TRACK_NAMES,
                                      precision="f32", device="cpu", row_stride=3)


def _compact_lib(model):
    quantiser = {"centroids": torch.zeros(2, 128), "codebooks": torch.zeros(16, 256, 8)}
    return library.FingerprintLibrary.from_codes(model, load_config(), quantiser, torch.zeros(14, dtype=torch.int32),
                                                 torch.zeros((14, 16), dtype=torch.uint8), FIRST, TRACK_NAMES,
                                                 precision="f32", device="cpu")


# ---- the rounding ---------------------------------------------------------------------------------------------------
def _torch_bits(x):
    return torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_numpy_rounding_equals_torch_bit_for_bit():
    rng = np.random.RandomState(3)
    random = (rng.randn(20000) * np.exp(rng.uniform(-30, 30, 20000))).astype(np.float32)
    any_bits = rng.randint(0, 2 ** 32, size=20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    any_bits = any_bits[~np.isnan(any_bits)]
    # ties: the 16 dropped bits are exactly 0x8000, after an even and after an odd kept mantissa; and one ulp to each side
    hi = rng.randint(0, 0x7F80, size=4000).astype(np.uint32) << 16
    ties = np.concatenate([hi | 0x8000, hi | 0x7FFF, hi | 0x8001, (hi | 0x8000) | 0x80000000]).view(np.float32)
    subnormal = np.concatenate([np.arange(0, 1 << 23, 4099, dtype=np.uint32),
                                np.array([1, 0x7FFF, 0x8000, 0x8001, 0x7FFFFF, 0x800000], np.uint32)]).view(np.float32)
    fmax = np.finfo(np.float32).max
    edge = np.array([fmax, -fmax, np.nextafter(fmax, 0), 3.3895314e38, 3.3961775e38, np.inf, -np.inf, 0.0, -0.0, 1.0,
                     1.00390625, 1.001953125, 1.005859375], np.float32)
    for name, x in (("random", random), ("any bits", any_bits), ("ties", ties), ("subnormal", subnormal), ("edge", edge)):
        got, want = bf16_bits(x), _torch_bits(x)
        assert got.dtype == np.uint16 and np.array_equal(got, want), (name, x[got != want][:5])
    assert bf16_bits(np.array([fmax], np.float32))[0] == 0x7F80          # the largest finite f32 rounds to +inf
    assert bf16_bits(np.array([1.00390625, 1.01171875], np.float32)).tolist() == [0x3F80, 0x3F82]   # ties go to even
    assert np.isnan(bf16_values(bf16_bits(np.array([np.nan, -np.nan], np.float32)))).all()   # (no fingerprint is one)
    # widening is exact and rounding is idempotent
    assert np.array_equal(bf16_values(bf16_bits(random)),
                          torch.from_numpy(random).to(torch.bfloat16).float().numpy())
    assert np.array_equal(bf16_bits(round_bf16(random)), bf16_bits(random))
    # the bound's premise: bf16 keeps 8 significant bits, so a component moves by at most 2^-8 relative (normal range)
    # -- and by more than 2^-9 for some, so no smaller power of two bounds a score's worst case
    normal = random[np.abs(random) > 1e-30].astype(np.float64)
    moved = np.abs(round_bf16(normal.astype(np.float32)).astype(np.float64) - normal) / np.abs(normal)
    assert (moved <= 2.0 ** -8).all() and moved.max() > 2.0 ** -9
    assert library.HALF_SCORE_BOUND == 2.0 ** -8


# ---- tables and files on the CPU --------------------------------------------------------------------------------------
def test_from_half_tables_on_the_cpu():
    model = _tiny_model()
    x = _f32_rows()
    lib = _half_lib(model, x)
    assert lib.is_half and not lib.is_compact and lib.row_stride == 1
    assert lib.n_rows == 14 and lib.n_tracks == 4 and lib.first.tolist() == FIRST and lib.names == TRACK_NAMES
    rows = lib.half_rows()
    assert rows.dtype == torch.bfloat16 and tuple(rows.shape) == (14, 128) and rows.is_contiguous()
    assert torch.equal(rows, torch.from_numpy(x).to(torch.bfloat16))
    assert np.array_equal(rows.float().numpy(), round_bf16(x))
    assert lib.nbytes == 14 * 256                                   # a CPU device: the library's own tensors only
    # bf16 tensors are taken as they are; anything else is refused
    same = library.FingerprintLibrary.from_half(model, load_config(), rows, FIRST, TRACK_NAMES, precision="f32",
                                                device="cpu")
    assert torch.equal(same.half_rows(), rows)
    for bad in (torch.from_numpy(x), torch.zeros((14, 64), dtype=torch.bfloat16), bf16_bits(x).astype(np.int32)):
        with pytest.raises(ValueError, match="half"):
            library.FingerprintLibrary.from_half(model, load_config(), bad, FIRST, TRACK_NAMES, device="cpu")
    with pytest.raises(ValueError, match="track table"):
        library.FingerprintLibrary.from_half(model, load_config(), rows, [0, 7, 13], None, device="cpu")
    # a library without rows has its form's empty tensor
    empty = library.FingerprintLibrary.from_half(model, load_config(), rows[:0], [0, 0], ["x"], device="cpu")
    assert empty.is_half and empty.half_rows().dtype == torch.bfloat16 and tuple(empty.half_rows().shape) == (0, 128)
    with pytest.raises(ValueError, match="no half library"):
        _flat_lib(model).half_rows()


def test_save_and_load_round_trip_with_the_exact_files(tmp_path):
    model = _tiny_model()
    x = _f32_rows()
    lib = _half_lib(model, x)
    out = str(tmp_path / "half")
    lib.save(out)
    assert sorted(os.listdir(out)) == ["library.json", "library_half.npy", "library_tracks.npy"]
    meta = json.load(open(os.path.join(out, "library.json")))
    assert meta["format"] == 5 == library.FORMAT_HALF and meta["n_rows"] == 14 and meta["names"] == TRACK_NAMES
    bits = np.load(os.path.join(out, "library_half.npy"))
    assert bits.dtype == np.uint16 and bits.shape == (14, 128) and np.array_equal(bits, bf16_bits(x))
    assert np.load(os.path.join(out, "library_tracks.npy")).tolist() == FIRST
    back = library.FingerprintLibrary.load(out, model)
    assert back.is_half and torch.equal(back.half_rows(), lib.half_rows()) and back.first.tolist() == FIRST
    assert back.names == lib.names and back.settings == lib.settings and back.precision == "f32"
    # another model is refused, as for the other forms
    other = _tiny_model()
    with torch.no_grad():
        next(other.parameters()).add_(1.0)
    with pytest.raises(ValueError, match="another model"):
        library.FingerprintLibrary.load(out, other)
    assert library.FingerprintLibrary.load(out, other, force=True).is_half
    # a table that does not cover the rows
    np.save(os.path.join(out, "library_tracks.npy"), np.array([0, 5], np.int64))
    with pytest.raises(ValueError, match="14 rows"):
        library.FingerprintLibrary.load(out, model)
    # format 4 was never written and is still refused by that name
    meta["format"] = 4
    json.dump(meta, open(os.path.join(out, "library.json"), "w"))
    with pytest.raises(ValueError, match="format 4"):
        library.FingerprintLibrary.load(out, model)


def test_the_truth_table_of_the_four_forms():
    model = _tiny_model()
    forms = {"flat": _flat_lib(model), "thin": _thin_lib(model), "compact": _compact_lib(model), "half": _half_lib(model)}
    assert {k: (v.is_compact, v.is_half) for k, v in forms.items()} == {
        "flat": (False, False), "thin": (False, False), "compact": (True, False), "half": (False, True)}
    assert ShardedFingerprintLibrary.split(forms["flat"], 2).is_half is False


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_a_half_library_refuses_what_needs_the_flat_form():
    model = _tiny_model()
    lib, wave = _half_lib(model), np.zeros(16000, np.float32)
    calls = {
        "rows()": lambda: lib.rows(),
        "identify(tempo=)": lambda: lib.identify(wave, tempo=0.05),
        "identify_windows(tempo=)": lambda: lib.identify_windows(wave, tempo=0.05),
        "match(tempo=)": lambda: lib.match(wave, tempo=0.05),
        "identify(query_stride=2)": lambda: lib.identify(wave, query_stride=2),
        "identify_windows(query_stride=2)": lambda: lib.identify_windows(wave, query_stride=2),
        "thin()": lambda: lib.thin(2),
        "compress()": lambda: lib.compress(),
        "self_matches()": lambda: lib.self_matches(),
        "self_matches(tempo=)": lambda: lib.self_matches(tempo=0.05),
        "halve()": lambda: lib.halve(),
        "build(index='half', row_stride=2)": lambda: library.FingerprintLibrary.build(model, [], load_config(),
                                                                                      index="half", row_stride=2),
        "split": lambda: ShardedFingerprintLibrary.split(lib, 2),
        "sharded constructor": lambda: ShardedFingerprintLibrary([lib]),
    }
    for what, call in calls.items():
        with pytest.raises(NotImplementedError, match="half") as err:
            call()
        assert len(str(err.value)) > 40, what                        # it says what to use instead
    # rows() points at what a half library does have
    with pytest.raises(NotImplementedError, match=r"half_rows\(\)"):
        lib.rows()
    from grafp_amd.monitor import StreamMonitor
    with pytest.raises(NotImplementedError, match="half"):
        StreamMonitor(lib, 1, query_stride=2)
    # query_stride = 1 is no stride: only the ordinary value check runs
    assert lib._need_stride_form("identify", 1) == 1
    with pytest.raises(ValueError, match="index must be"):
        library.FingerprintLibrary.build(model, [], load_config(), index="quarter")


def test_the_other_forms_keep_their_refusals():
    model = _tiny_model()
    with pytest.raises(NotImplementedError, match="needs the flat form of a library \\(f32 rows\\): this one is compact"):
        _compact_lib(model).rows()
    with pytest.raises(NotImplementedError, match="needs every row of a track: this library keeps every 3th"):
        _thin_lib(model).thin(2)
    with pytest.raises(NotImplementedError, match="needs every row of a track"):
        _thin_lib(model).halve()
    with pytest.raises(NotImplementedError, match="is compact"):
        _compact_lib(model).halve()
    assert _flat_lib(model).rows().dtype == torch.float32


def test_ops_check_the_rows_before_they_ask_for_a_device():
    rows = torch.zeros((6, 128), dtype=torch.bfloat16)
    ids, first = torch.zeros((3, 2), dtype=torch.int64), torch.tensor([0, 6])
    item = (torch.zeros(1, dtype=torch.int64), torch.full((1,), 3, dtype=torch.int32))
    for bad in (rows.float(), rows[:, :64], rows.t().contiguous().t(), rows.view(torch.int16)):
        with pytest.raises(ValueError, match="torch.bfloat16"):
            ops.identify_half(bad, first, torch.zeros(3, 128), ids, *item)
        with pytest.raises(ValueError, match="torch.bfloat16"):
            ops.cross_match_half(bad, first, torch.zeros(3, 128), torch.tensor([0, 3]), ids)
        with pytest.raises(ValueError, match="torch.bfloat16"):
            ops.search_l2_half(bad, torch.zeros(6), torch.zeros(3, 128), 2)
    # the flat siblings' checks, under the half op's name
    with pytest.raises(ValueError, match="identify_half: top=65"):
        ops.identify_half(rows, first, torch.zeros(3, 128), ids, *item, top=65)
    with pytest.raises(ValueError, match="cross_match_half.*source table"):
        ops.cross_match_half(rows, first, torch.zeros(3, 128), torch.tensor([0, 2]), ids)
    # and then: no CPU
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.identify_half(rows, first, torch.zeros(3, 128), ids, *item)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.cross_match_half(rows, first, torch.zeros(3, 128), torch.tensor([0, 3]), ids)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.search_l2_half(rows, torch.zeros(6), torch.zeros(3, 128), 2)


# ---- routing ----------------------------------------------------------------------------------------------------------
def test_the_hooks_route_a_half_library_to_the_half_ops(monkeypatch):
    """A half library's hooks launch ops.identify_half and ops.cross_match_half on its bf16 tensor and its index is an
    ops.HalfL2Index over that very tensor; a flat library takes the calls it took before."""
    model = _tiny_model()
    half, flat = _half_lib(model), _flat_lib(model)
    id_args = (torch.zeros(3, 128), torch.zeros((3, 2), dtype=torch.int64), np.zeros(1, np.int64), np.full(1, 3, np.int32),
               5, None, 3)
    kw = dict(top=8, min_votes=4, min_overlap=1)
    m_args = (torch.zeros(3, 128), torch.tensor([0, 3]), torch.zeros((3, 2), dtype=torch.int64), None, kw)
    for lib, id_op, m_op, rows in ((half, "identify_half", "cross_match_half", half.half_rows()),
                                   (flat, "identify", "cross_match", flat.rows())):
        seen = []
        others = {"identify", "identify_half", "identify_pq", "identify_thin", "cross_match", "cross_match_half",
                  "cross_match_pq"} - {id_op, m_op}
        for name in others:
            monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the wrong op was launched"))
        monkeypatch.setattr(ops, id_op, lambda *a, **k: seen.append(("id", a, k)) or "identified")
        monkeypatch.setattr(ops, m_op, lambda *a, **k: seen.append(("match", a, k)) or "matched")
        assert lib._identify_lists(*id_args) == "identified" and lib._match_launch(*m_args) == "matched"
        (_, a, k), (_, b, kb) = seen
        assert a[0] is rows and len(a) == 6 and k == dict(top=5, min_overlap=None, max_len=3)
        assert b[0] is rows and len(b) == 5 and kb == kw
        monkeypatch.undo()

    class FakeIndex:
        made = []

        def __init__(self, d=128, device=None):
            self.added, self.asked = [], []
            FakeIndex.made.append(self)

        def add(self, x):
            self.added.append(x)

        def search(self, q, k):
            self.asked.append((q, k))
            return None, "ids"

    monkeypatch.setattr(ops, "HalfL2Index", FakeIndex)
    monkeypatch.setattr(ops, "FlatL2Index", lambda **k: pytest.fail("a half library made a flat index"))
    q = torch.zeros(3, 128)
    assert half._search_rows(q, 20) == "ids" and half._search_rows(q, 5) == "ids"
    assert len(FakeIndex.made) == 1 and len(FakeIndex.made[0].added) == 1
    assert FakeIndex.made[0].added[0] is half.half_rows()            # one bf16 tensor, shared
    assert [k for _, k in FakeIndex.made[0].asked] == [14, 5]


def test_the_command_line_knows_the_half_form():
    from grafp_amd import identify
    with pytest.raises(SystemExit) as err:
        identify.main(["build", "--ckp", "x", "--source", "y", "--out", "z", "--index", "third"])
    assert err.value.code == 2
    assert "--index flat|ivfpq|half" in identify.__doc__


# ---- the shipped objects ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernels", [("identify_half", ["identify_half_kernel", "identify_half_kernel"]),
                                          ("crossmatch_half", ["cross_match_half_kernel",
                                                               "cross_match_half_plan_kernel"])])
def test_half_kernels_have_no_packed_f32_instructions(name, kernels):
    """The shipped object's own command (make -n), compiled to device assembly: the expected kernels are there and none
    holds a packed-f32 instruction."""
    asm = shipped_asm(name)
    found = re.findall(r"^(_ZN5grafp\w+):", asm, flags=re.M)
    assert len(found) == len(kernels) and sorted(re.match(r"_ZN5grafp\d+([a-z_]+?)(?:ILb|E)", f).group(1)
                                                 for f in found) == sorted(kernels), found
    assert not re.search(r"^\s*v_pk_\w+_f32", asm, flags=re.M)
    assert "v_fmac_f32" in asm or "v_fma_f32" in asm
    assert re.search(r"v_lshlrev_b32|v_and_b32", asm)               # the rows are widened in registers
