"""Writes tests/golden/gemm_plan.json: what the plan queries of csrc/gemm.hip (pure host functions) answer for a table
of shapes, recorded from a library built from the commit BEFORE a change to that file; tests/test_gemm_cpu.py asserts
that the library of the checkout still answers the same.

    python tests/golden/make_gemm_plan.py PATH_TO_libgrafp_hip.so
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gemm_plan.json")
# S, L, N32, N64, N128, XL (GM_CFG_* of gemm.hip): every tile configuration the rule of gemm_plan can choose
RULE_CONFIGS = {0, 1, 2, 3, 4, 5}
# SHAPES of tests/test_gpu_gemm.py
GPU_TEST_SHAPES = [(64, 64, 1, 8192, 2), (256, 64, 1, 8192, 2), (64, 256, 1, 8192, 2), (128, 128, 4, 4096, 2),
                   (128, 64, 1, 2048 * 3, 1), (512, 2048, 1, 1024, 2), (2048, 512, 1, 1024, 1), (256, 768, 1, 2560, 2),
                   (1024, 1024, 4, 2048, 2), (96, 32, 1, 1280, 1), (64, 64, 1, 128 * 2 * 37, 2),
                   (64, 256, 1, 131072, 2), (128, 128, 4, 131072, 2), (128, 512, 1, 262144, 2), (96, 160, 1, 524288, 1),
                   (64, 64, 1, 2 * 512 * 131, 2), (32, 96, 1, 65536, 1),
                   (256, 512, 1, 2 * 256 * 9, 2), (512, 1280, 1, 256 * 7, 1), (512, 512, 1, 256, 1),
                   (256, 2560, 1, 2 * 256 * 33, 2)]
# what grafp_conv1x1_gemm_supported refuses: K = 8 (the stem), columns per view not a multiple of 128, rows per group
# not a multiple of 32, K per group not a multiple of 32, groups that do not divide, columns that the views do not divide
UNSUPPORTED = [(64, 8, 1, 1024, 1), (64, 64, 1, 1000, 1), (80, 64, 2, 1024, 1), (128, 96, 2, 1024, 1), (96, 64, 5, 1024, 1),
               (64, 64, 1, 1024 + 128, 2), (0, 64, 1, 1024, 1), (64, 64, 1, 1024, 0)]


def shapes():
    """[(R, K, groups, M, views)]: every layer of the encoder as tools/gemm_bench.py runs it (forward, data gradient,
    concatenated operand: K includes the second operand's rows) at 128, 512, 2048 and 4096 clip-views as one view and as
    two, the shapes of tests/test_gpu_gemm.py, and the per-configuration shapes of its partials test."""
    out = []
    for C, N in ((64, 1024), (128, 512), (256, 256), (512, 128)):
        layers = ((C, C, 1), (2 * C, 2 * C, 4), (C, 2 * C, 1), (4 * C, C, 1), (C, 4 * C, 1),          # forward
                  (C, C + C, 1), (2 * C, 2 * C, 4), (2 * C, C, 1), (C, 4 * C + C, 1), (4 * C, C, 1))  # data gradients
        for R, K, g in layers:
            for clips in (128, 512, 2048, 4096):
                for views in (1, 2):
                    out.append((R, K, g, clips * N, views))
    out += GPU_TEST_SHAPES
    out += [(64, 64, 1, 256, 2), (512, 64, 1, 512, 1), (256, 512, 1, 512, 2), (32, 32, 1, 65536, 1), (64, 64, 1, 65536, 1),
            (128, 512, 1, 131072, 1)]
    return list(dict.fromkeys(out))


def bind(lib):
    i, l = ctypes.c_int, ctypes.c_int64
    lib.grafp_conv1x1_gemm_supported.restype, lib.grafp_conv1x1_gemm_supported.argtypes = i, [i, i, i, l, i]
    lib.grafp_conv1x1_gemm_partials.restype, lib.grafp_conv1x1_gemm_partials.argtypes = i, [i, i, i, l, i]
    lib.grafp_conv1x1_gemm_plan.restype, lib.grafp_conv1x1_gemm_plan.argtypes = i, [i, i, i, l, i, ctypes.c_void_p]
    return lib


def query(lib, shape):
    """One row of the file: the answers of the three queries for a shape (info: null where the shape is refused)."""
    ok = lib.grafp_conv1x1_gemm_supported(*shape)
    info = (ctypes.c_int * 8)()
    rc = lib.grafp_conv1x1_gemm_plan(*shape, info)
    assert (rc == 0) == bool(ok), shape
    return {"shape": list(shape), "supported": ok, "partials": lib.grafp_conv1x1_gemm_partials(*shape),
            "info": list(info) if ok else None}


def main(path):
    import torch  # noqa: F401  -- first: the library binds to the HIP runtime torch ships (grafp_amd/_lib.py)
    lib = bind(ctypes.CDLL(path))
    rows = [query(lib, s) for s in shapes() + UNSUPPORTED]
    assert all(r["supported"] for r in rows[:-len(UNSUPPORTED)]) and not any(r["supported"] for r in rows[-len(UNSUPPORTED):])
    seen = {r["info"][0] for r in rows if r["supported"]}
    assert seen == RULE_CONFIGS, f"configurations the table reaches: {sorted(seen)}"
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} shapes -> {OUT} ({os.path.getsize(OUT)} bytes); configurations {sorted(seen)}")


if __name__ == "__main__":
    main(sys.argv[1])
