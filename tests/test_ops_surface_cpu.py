"""The public surface of ``selfrec_amd.ops`` without a GPU: every name, signature and constant recorded in
tests/golden/ops_surface.json (taken from the single-file front end before it became a package) is still there and
unchanged, ``__all__`` is sound, and every ``ops.<name>`` written in the repository resolves.  The recorded surface may gain
names; it never loses or alters one."""
import ast
import inspect
import json
import os
import re
import subprocess
import types

import torch

from tests.test_shapes_cpu import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE = os.path.join(GOLDEN, "ops_surface.json")
# what __all__ lacked while the rest of the repository called it as ops.<name>
ADDED_TO_ALL = ("make_epilogue", "bpr_ws", "scalar_ws", "infonce_plan", "l2_reg_fwd", "l2_reg_bwd", "batch_fetch_args",
                "topk_trim_mark_ties", "find_k_largest_host", "gather_floor_probe", "spmm_gather_bound",
                "seq_embed_supported", "kmeans_split", "gpu_available")


def _sig(f):
    try:
        return str(inspect.signature(f))
    except (TypeError, ValueError):
        return None


def describe(mod):
    """{name: record} of the public attributes of ``mod``; modules (numpy, torch, ... and the package's own submodules)
    and ``from __future__`` features are imports, not surface."""
    out = {}
    for name in sorted(vars(mod)):
        v = getattr(mod, name)
        if name.startswith("_") or isinstance(v, types.ModuleType) or type(v).__name__ == "_Feature":
            continue
        if isinstance(v, type) and issubclass(v, torch.autograd.Function):
            rec = {"kind": "autograd", "forward": _sig(v.forward), "backward": _sig(v.backward),
                   "bases": [b.__name__ for b in v.__mro__[1:] if b.__module__.startswith("selfrec_amd")]}
        elif isinstance(v, type):
            methods = {m: _sig(f) for m, f in sorted(vars(v).items()) if not m.startswith("_") and callable(f)}
            rec = {"kind": "class", "signature": _sig(v), "methods": methods}
        elif callable(v):
            rec = {"kind": "function", "signature": _sig(v)}
        else:
            rec = {"kind": "constant", "value": json.loads(json.dumps(v))}
        out[name] = rec
    return out


def test_every_recorded_name_is_there_unchanged():
    from selfrec_amd import ops
    with open(SURFACE) as f:
        want = json.load(f)
    got = describe(ops)
    assert len(want) >= 133
    for name, rec in want.items():
        assert name in got, f"ops.{name} is gone"
        if rec["kind"] == "autograd":            # a shared base may join the chain; none may leave it
            assert set(rec["bases"]) <= set(got[name]["bases"]), name
            rec, have = dict(rec, bases=None), dict(got[name], bases=None)
        else:
            have = got[name]
        assert have == rec, f"ops.{name}: {have} != {rec}"
    assert ops._lib.load and ops.require_gpu is ops._lib.require_gpu


def test_all_is_sound_and_star_import_works():
    from selfrec_amd import ops
    names = ops.__all__
    assert len(names) == len(set(names))
    assert "sumsq" not in names
    for name in names:
        assert hasattr(ops, name), name
    for name in ADDED_TO_ALL:
        assert name in names and callable(getattr(ops, name)), name
    ns = {}
    exec("from selfrec_amd.ops import *", ns)
    assert all(ns[name] is getattr(ops, name) for name in names)


def test_init_holds_imports_and_all_only_and_no_submodule_is_long():
    from selfrec_amd import ops
    pkg = os.path.dirname(ops.__file__)
    with open(os.path.join(pkg, "__init__.py")) as f:
        body = ast.parse(f.read()).body
    for node in body:
        is_doc = isinstance(node, ast.Expr) and isinstance(node.value, ast.Constant) and isinstance(node.value.value, str)
        is_all = isinstance(node, ast.Assign) and [getattr(t, "id", None) for t in node.targets] == ["__all__"]
        assert is_doc or is_all or isinstance(node, (ast.Import, ast.ImportFrom)), ast.dump(node)[:80]
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as f:
                assert sum(1 for _ in f) <= 460, name


def _tracked_python_files():
    try:
        out = subprocess.run(["git", "ls-files", "*.py"], cwd=REPO, capture_output=True, text=True, check=True).stdout.split()
        if out:
            return out
    except (OSError, subprocess.CalledProcessError):
        pass
    with open(os.path.join(REPO, ".gitignore")) as f:        # (an exported tree without its history: every .py in it
        skip = {line.strip().rstrip("/").split("/")[-1] for line in f if line.strip().endswith("/")}   # but .gitignore's dirs)
    found = []
    for root, dirs, files in os.walk(REPO):
        dirs[:] = [d for d in dirs if d not in skip and not d.startswith(".")]
        found += [os.path.relpath(os.path.join(root, f), REPO) for f in files if f.endswith(".py")]
    return found


def test_every_ops_name_written_in_the_repository_resolves():
    from selfrec_amd import ops
    pat = re.compile(r"(?<!\w)(?:ops|_real_ops)\.([A-Za-z_]\w*)")
    probe = re.compile(r"""(?:has|get|set)attr\(\s*(?:\w+\.)?(?:ops|_real_ops)\s*,\s*["'](\w+)["']""")   # the string probes
    used = {}
    for path in _tracked_python_files():
        with open(os.path.join(REPO, path), encoding="utf-8", errors="replace") as f:
            src = f.read()
        for name in pat.findall(src) + probe.findall(src):
            used.setdefault(name, path)
    assert "_segments" in used                               # (engine.py asks for it by name to tell the CPU stand-in apart)
    assert len(used) >= 115                                  # (the scan sees the repository: 119 names when this was written)
    missing = {name: path for name, path in used.items() if not hasattr(ops, name)}
    assert not missing, missing


def test_patching_the_package_reaches_its_callers():
    """the six names tests and tools assign to (ops.<name> = ...) are read through the package by the product, and the one
    in-package caller among them, spmm_probe, lives beside its callee spmm_plan_run_tasks"""
    from selfrec_amd import ops
    six = ("spmm_probe", "spmm_set_xcd_shares", "spmm_plan_run_tasks", "bpr_infonce", "adam_step", "column_class_order")
    assert ops.spmm_probe.__module__ == ops.spmm_plan_run_tasks.__module__
    pkg = os.path.dirname(ops.__file__)
    for fname in sorted(os.listdir(pkg)):
        if not fname.endswith(".py") or fname == "__init__.py":
            continue
        with open(os.path.join(pkg, fname)) as f:
            tree = ast.parse(f.read())
        defined = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
        called = {n.func.id for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)}
        assert not (called & set(six)) - defined, f"{fname} calls {sorted((called & set(six)) - defined)} by bare name"
