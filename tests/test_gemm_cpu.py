"""CPU test of the launch plan of csrc/gemm.hip: the three plan queries (pure host functions: no GPU) answer what the
library of the commit before the kernels' shared parts were written once answered, over every layer shape of the encoder
and the shapes of the GPU tests (tests/golden/gemm_plan.json, written by tests/golden/make_gemm_plan.py)."""
import importlib.util
import json
import os

from _common import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_gemm_plan", os.path.join(GOLDEN, "make_gemm_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plans_are_the_recorded_ones():
    from grafp_amd._lib import lib
    mk = _maker()
    with open(os.path.join(GOLDEN, "gemm_plan.json")) as f:
        rows = json.load(f)
    assert [tuple(r["shape"]) for r in rows] == mk.shapes() + mk.UNSUPPORTED
    for want in rows:
        assert mk.query(lib, tuple(want["shape"])) == want, want["shape"]
    # the table reaches every tile configuration the rule can choose
    assert {r["info"][0] for r in rows if r["supported"]} == mk.RULE_CONFIGS
    # its copy of the GPU tests' shapes is the list of tests/test_gpu_gemm.py
    spec = importlib.util.spec_from_file_location("test_gpu_gemm", os.path.join(ROOT, "tests", "test_gpu_gemm.py"))
    gpu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gpu)
    assert gpu.SHAPES == mk.GPU_TEST_SHAPES


def test_unsupported_shapes_are_still_refused():
    from grafp_amd._lib import lib
    mk = _maker()
    for shape in mk.UNSUPPORTED:
        assert lib.grafp_conv1x1_gemm_supported(*shape) == 0, shape
        assert lib.grafp_conv1x1_gemm_partials(*shape) == 0, shape
        assert lib.grafp_conv1x1_gemm_plan(*shape, None) == -1 and b"conv1x1_gemm_plan" in lib.grafp_last_error(), shape
