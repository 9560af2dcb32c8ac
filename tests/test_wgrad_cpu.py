"""CPU test of the launch plans of csrc/wgrad.hip: the plan and workspace queries (pure host functions: no GPU) answer
what the library of the commit before the kernels' shared parts were written once answered, over every layer shape of
the encoder and the odd shapes of the GPU tests (tests/golden/wgrad_plan.json, written by tests/golden/make_wgrad_plan.py)."""
import importlib.util
import json
import os

from _common import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_wgrad_plan", os.path.join(GOLDEN, "make_wgrad_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plans_and_workspaces_are_the_recorded_ones():
    from grafp_amd._lib import lib
    mk = _maker()
    with open(os.path.join(GOLDEN, "wgrad_plan.json")) as f:
        rows = json.load(f)
    assert [tuple(r["shape"]) for r in rows] == mk.shapes()
    for want in rows:
        assert mk.query(lib, tuple(want["shape"])) == want, want["shape"]
    # the table reaches every configuration the rule can choose, and a forced T128 / S128 that has to fall back
    assert {r["info"][0] for r in rows} == mk.RULE_CONFIGS
    # (81 x 64 columns: 8 slices of whole 64-column chunks; whole 128-column chunks would make 7)
    by_shape = {tuple(r["shape"]): r["tile_ws"] for r in rows}
    for shape, wide, narrow in (((512, 512, 1, 5184, 1), 8, 0), ((1024, 1024, 1, 5184, 1), 10, 1)):
        ws = by_shape[shape]
        assert ws[mk.TILES.index(wide)] == ws[mk.TILES.index(narrow)] == 8 * shape[0] * shape[1] * 4
