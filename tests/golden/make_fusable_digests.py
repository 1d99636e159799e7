#!/usr/bin/env python3
"""Prints the two digests selfrec_amd/dropin.py keeps per fusable reference model file: SHA-256 of the bytes and of the
canonical syntax dump (comments, blank lines, indentation style and docstrings do not enter it).  Run in the build container:
    python tests/golden/make_fusable_digests.py REFERENCE_CHECKOUT [--json tests/golden/reference_model_files.json]
With --json it also writes, per file, the two digests, the modules and names it imports and the bases of its model class:
what tests/test_host_logic.py holds dropin.py's table and the mirrored import paths to.
Facts about the reference's files, not copies of them."""
import ast
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from selfrec_amd.dropin import syntax_digest  # noqa: E402

NAMES = ("XSimGCL", "LightGCN", "SimGCL", "SGL", "MF")


def facts(name, src):
    tree = ast.parse(src.decode())
    imports = []
    for node in tree.body:
        if isinstance(node, ast.Import):
            imports += [{"import": a.name, "as": a.asname} for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            imports.append({"from": node.module, "names": [a.name for a in node.names]})
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)
    return {"sha256": hashlib.sha256(src).hexdigest(), "syntax_sha256": syntax_digest(src.decode()), "imports": imports,
            "bases": [ast.unparse(b) for b in cls.bases]}


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--json" in args:
        k = args.index("--json")
        out = args[k + 1]
        del args[k:k + 2]
    if len(args) != 1:
        raise SystemExit(__doc__)
    root = args[0]
    table = {}
    for name in NAMES:
        src = open(os.path.join(root, "model", "graph", name + ".py"), "rb").read()
        table[name] = facts(name, src)
        print(f'    "{name}": ("{table[name]["sha256"]}",\n               "{table[name]["syntax_sha256"]}"),')
    if out:
        with open(out, "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")
