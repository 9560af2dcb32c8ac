"""Writes tests/golden/wgrad_plan.json: what the weight-gradient plan queries of csrc/wgrad.hip (pure host functions)
answer for a table of shapes, recorded from a library built from the commit BEFORE a change to that file;
tests/test_wgrad_cpu.py asserts that the library of the checkout still answers the same.

    python tests/golden/make_wgrad_plan.py PATH_TO_libgrafp_hip.so
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "wgrad_plan.json")
TILES = list(range(-1, 11))
# the configurations the rule of wgrad_dma_plan can choose (-1: no LDS-DMA plan, the register-staged kernel)
RULE_CONFIGS = {-1, 0, 1, 5, 6, 7, 8, 10}


def shapes():
    """[(Cout, Cin, groups, M, views)]: every layer of the encoder (the list of tools/gemm_bench.py --wgrad) at 128, 512,
    2048 and 4096 clip-views as one view and as two, the ragged and odd shapes of tests/test_gpu_gemm.py, and what the
    assertions of main() need beyond those."""
    out = []
    for C, N in ((64, 1024), (128, 512), (256, 256), (512, 128)):
        for co, ci, g in ((C, C, 1), (2 * C, 2 * C, 4), (C, 2 * C, 1), (4 * C, C, 1), (C, 4 * C, 1)):
            for clips in (128, 512, 2048, 4096):
                for views in (1, 2):
                    out.append((co, ci, g, clips * N, views))
    out += [(40, 24, 1, 777, 1), (96, 192, 4, 1000, 1), (96, 160, 1, 1280, 1), (320, 256, 1, 4160, 1), (256, 512, 1, 64, 1)]
    # L32 (5): a grouped convolution with 256 rows per group between 400 and 750 MB of operands -- the encoder's only one
    # (stage 3) is there between 763 and 1430 clip-views; this is its first M with whole 64-column chunks
    out.append((1024, 1024, 4, 97664, 1))
    # 81 x 64 columns with 8 slices wanted: whole 64-column chunks give 8 slices of 704 columns, whole 128-column chunks
    # would give 7 of 768 -- the workspace shows whether a forced T128 / S128 fell back to T / S
    out += [(512, 512, 1, 5184, 1), (1024, 1024, 1, 5184, 1)]
    return out


def bind(lib):
    i, l, z = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    lib.grafp_conv1x1_wgrad_plan.restype, lib.grafp_conv1x1_wgrad_plan.argtypes = i, [i, i, i, l, i, ctypes.c_void_p]
    lib.grafp_conv1x1_wgrad_tile_workspace.restype, lib.grafp_conv1x1_wgrad_tile_workspace.argtypes = z, [i, i, i, l, i, i]
    lib.grafp_conv1x1_wgrad_pro_workspace.restype, lib.grafp_conv1x1_wgrad_pro_workspace.argtypes = z, [i, i, i, l, i]
    lib.grafp_conv1x1_wgrad_workspace.restype, lib.grafp_conv1x1_wgrad_workspace.argtypes = z, [i, i, i, l]
    lib.grafp_conv1x1_wgrad_f32_workspace.restype, lib.grafp_conv1x1_wgrad_f32_workspace.argtypes = z, [i, i, i, l]
    return lib


def query(lib, shape):
    """One row of the file: the answers of the five queries for a shape."""
    co, ci, g, M, views = shape
    info = (ctypes.c_int * 8)()
    assert lib.grafp_conv1x1_wgrad_plan(co, ci, g, M, views, info) == 0, shape
    return {"shape": list(shape), "info": list(info),
            "tile_ws": [lib.grafp_conv1x1_wgrad_tile_workspace(co, ci, g, M, views, t) for t in TILES],
            "pro_ws": lib.grafp_conv1x1_wgrad_pro_workspace(co, ci, g, M, views),
            "ws": lib.grafp_conv1x1_wgrad_workspace(co, ci, g, M),
            "f32_ws": lib.grafp_conv1x1_wgrad_f32_workspace(co, ci, g, M)}


def main(path):
    import torch  # noqa: F401  -- first: the library binds to the HIP runtime torch ships (grafp_amd/_lib.py)
    lib = bind(ctypes.CDLL(path))
    rows = [query(lib, s) for s in shapes()]
    seen = {r["info"][0] for r in rows}
    assert seen == RULE_CONFIGS, f"configurations the table reaches: {sorted(seen)}"
    by_shape = {tuple(r["shape"]): r for r in rows}
    for shape, wide, narrow in (((512, 512, 1, 5184, 1), 8, 0), ((1024, 1024, 1, 5184, 1), 10, 1)):
        r, n = by_shape[shape], shape[0] * shape[1] * 4
        assert (shape[3] // shape[4]) % 128 == 64
        assert r["tile_ws"][TILES.index(wide)] == r["tile_ws"][TILES.index(narrow)] == 8 * n, (shape, r["tile_ws"])
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} shapes -> {OUT} ({os.path.getsize(OUT)} bytes); configurations {sorted(seen)}")


if __name__ == "__main__":
    main(sys.argv[1])
