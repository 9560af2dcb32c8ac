"""Bits of the normalise-on-load (PRO) products and weight gradients of the library in GRAFP_HIP_LIB (or the package's own):
one line `form | shape | tensor | sha256` per output tensor, from seeded operands drawn on the device.

    GRAFP_HIP_LIB=<parent build> python tools/pro_bits.py --out a.txt
    python tools/pro_bits.py --out b.txt
    python tools/pro_bits.py --compare a.txt b.txt        # table per form, exit status 1 if any tensor differs

The lists are those of profiles/gemm_refactor_ab.txt (PRO, PRO + STATS, weight gradient with a pro_tab, and the plain forms
beside them) plus every (weight-gradient tile, activation code) pair: each is a kernel of its own since the activation
code became a template argument (profiles/pro_cost_bits.txt)."""
import argparse, hashlib, os, sys
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (R, K, groups, M, views): SHAPES of tests/test_gpu_gemm.py and one shape per tile configuration (S, L, XL -> L with a
# pro_tab, N32, N64, N128)
PRODUCTS = [(64, 64, 1, 8192, 2), (256, 64, 1, 8192, 2), (64, 256, 1, 8192, 2), (128, 128, 4, 4096, 2),
            (128, 64, 1, 2048 * 3, 1), (512, 2048, 1, 1024, 2), (2048, 512, 1, 1024, 1), (256, 768, 1, 2560, 2),
            (1024, 1024, 4, 2048, 2), (96, 32, 1, 1280, 1), (64, 64, 1, 128 * 2 * 37, 2),
            (64, 256, 1, 131072, 2), (128, 128, 4, 131072, 2), (128, 512, 1, 262144, 2), (96, 160, 1, 524288, 1),
            (64, 64, 1, 2 * 512 * 131, 2), (32, 96, 1, 65536, 1),
            (256, 512, 1, 2 * 256 * 9, 2), (512, 1280, 1, 256 * 7, 1), (512, 512, 1, 256, 1), (256, 2560, 1, 2 * 256 * 33, 2),
            (64, 64, 1, 256, 2), (512, 64, 1, 512, 1), (256, 512, 1, 512, 2), (32, 32, 1, 65536, 1), (64, 64, 1, 65536, 1),
            (128, 512, 1, 131072, 1)]
# (cout, cin, groups, M, views)
WGRADS = [(96, 160, 1, 1280, 1), (512, 1024, 4, 1024, 2), (256, 512, 1, 64, 1), (64, 64, 1, 8192, 2), (128, 128, 4, 8192, 2),
          (1024, 256, 1, 2048, 2), (64, 256, 1, 262144, 2), (128, 256, 1, 524288, 1)]
WG_PRO_TILES = [0, 1, 2, 3, 4, 5, 8, 10]          # T, S, L, S32, M32, L32, T128, S128
WG_TILE_SHAPES = [(96, 160, 1, 1280, 1), (512, 1024, 4, 1024, 2), (64, 128, 1, 8192, 2)]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def run(out):
    from grafp_amd import ops
    dev = "cuda:0"
    lines = []

    def put(form, shape, name, t):
        lines.append(f"{form} | {shape} | {name} | {sha(t)}")

    for i, shape in enumerate(PRODUCTS):
        R, K, groups, M, views = shape
        torch.manual_seed(1000 + i)
        w = (torch.randn(R, K // groups, device=dev) * 0.2).to(torch.bfloat16)
        x = (torch.randn(K, M, device=dev) * 2.0 + 1.0).to(torch.bfloat16)
        tab = torch.stack((torch.rand(K, views, device=dev) + 0.5, torch.randn(K, views, device=dev)), dim=-1).contiguous()
        put("plain", shape, "y", ops.conv1x1_gemm(w, x, groups, views))
        y, part = ops.conv1x1_gemm(w, x, groups, views, stats=True)
        put("STATS", shape, "y", y)
        put("STATS", shape, "part", part)
        if K // groups > 1024:
            continue
        for act in (i % 3, (i + 1) % 3):                  # two of the three codes per shape, all three over the list
            put("PRO", shape, f"y act{act}", ops.conv1x1_gemm(w, x, groups, views, pro_tab=tab, pro_act=act, pro_slope=0.2))
            y, part = ops.conv1x1_gemm(w, x, groups, views, pro_tab=tab, pro_act=act, pro_slope=0.2, stats=True)
            put("PRO+STATS", shape, f"y act{act}", y)
            put("PRO+STATS", shape, f"part act{act}", part)

    def wg_case(i, shape):
        cout, cin, groups, M, views = shape
        torch.manual_seed(2000 + i)
        g = torch.randn(cout, M, device=dev).to(torch.bfloat16)
        x = (torch.randn(cin, M, device=dev) * 1.5 + 0.5).to(torch.bfloat16)
        tab = torch.stack((torch.rand(cin, views, device=dev) + 0.5, torch.randn(cin, views, device=dev)), dim=-1).contiguous()
        return g, x, tab

    for i, shape in enumerate(WGRADS):
        cout, cin, groups, M, views = shape
        g, x, tab = wg_case(i, shape)
        put("wgrad plain", shape, "dw", ops._wgrad_bf16(g, x, cout, cin, groups, M, may_defer=False))
        for act in (1, 2):
            put("wgrad with pro_tab", shape, f"dw act{act}",
                ops._wgrad_bf16(g, x, cout, cin, groups, M, views, tab, act, 0.2, may_defer=False))
    for i, shape in enumerate(WG_TILE_SHAPES):
        cout, cin, groups, M, views = shape
        g, x, tab = wg_case(100 + i, shape)
        for tile in WG_PRO_TILES:
            put("wgrad plain, tile forced", shape, f"dw tile{tile}",
                ops._wgrad_bf16(g, x, cout, cin, groups, M, views, tile=tile, may_defer=False))
            for act in (0, 1, 2):
                put("wgrad with pro_tab, tile forced", shape, f"dw tile{tile} act{act}",
                    ops._wgrad_bf16(g, x, cout, cin, groups, M, views, tab, act, 0.2, tile=tile, may_defer=False))
    torch.cuda.synchronize()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} tensors -> {out}")


def compare(a, b):
    def read(p):
        d = OrderedDict()
        for line in open(p):
            form, shape, name, h = [s.strip() for s in line.split("|")]
            d[(form, shape, name)] = h
        return d
    da, db = read(a), read(b)
    forms = OrderedDict()
    for key in da:
        n, bad = forms.get(key[0], (0, 0))
        forms[key[0]] = (n + 1, bad + (db.get(key) != da[key]))
    print("| form | tensors | differ |\n|---|---|---|")
    for form, (n, bad) in forms.items():
        print(f"| {form} | {n} | {bad} |")
    total, bad = sum(n for n, _ in forms.values()), sum(b_ for _, b_ in forms.values())
    missing = len(set(da) ^ set(db))
    print(f"| all | {total} | {bad} |")
    if missing:
        print(f"{missing} tensors are in one list only")
    for key in da:
        if db.get(key) != da[key]:
            print("differs:", key)
    return 1 if bad or missing else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    run(a.out or "pro_bits.txt")
