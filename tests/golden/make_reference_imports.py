"""Writes tests/golden/reference_imports.json: which project modules and names the reference's entry scripts import
(train.py, test_fp.py, generate.py, eval.py), read with `ast` -- names only, no code.
tests/test_host_cpu.py builds a stand-in checkout from it and imports that through grafp_amd.dropin.

    python tests/golden/make_reference_imports.py PATH_TO_A_CHECKOUT_OF_THE_REFERENCE
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SCRIPTS = ("train.py", "test_fp.py", "generate.py", "eval.py")


def project_imports(ref, fname):
    """[[module, [names] or None], ...] in source order: `from M import a, b` -> [M, [a, b]], `import M` -> [M, None];
    only modules that resolve inside the checkout, plus `faiss` (bound by grafp_amd.dropin)."""
    with open(os.path.join(ref, fname)) as f:
        tree = ast.parse(f.read())
    top = {n.split(".")[0] for n in os.listdir(ref)} | {"faiss"}
    out = []
    for node in tree.body:
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] in top:
            out.append([node.module, [a.name for a in node.names]])
        elif isinstance(node, ast.Import):
            out.extend([a.name, None] for a in node.names if a.name.split(".")[0] in top)
    return out


def main(ref):
    data = {fname: project_imports(ref, fname) for fname in SCRIPTS}
    with open(os.path.join(HERE, "reference_imports.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in data.items()) + "\n}\n")


if __name__ == "__main__":
    main(sys.argv[1])
