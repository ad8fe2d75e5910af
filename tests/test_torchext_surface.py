"""CPU-only pin of the public surface of `connecting_the_dots_amd.torchext` (no GPU, no built library): the names,
signatures, docstrings and constants of `torchext.functions` against tests/golden/torchext_surface.json (written by
tests/golden/make_torchext_surface.py), the names `torchext` itself exports, and the layering of the modules under it."""
import ast
import importlib.util
import json
import os
import pkgutil
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TORCHEXT = os.path.join(ROOT, "connecting_the_dots_amd", "torchext")

MODULE_CLASSES = {"CoordConv2d", "DispToDepth", "DisparityLoss", "LCN", "MultiScalePatternSimilarityLoss",
                  "ProjectionDepthSimilarityLoss", "RectifiedPatternSimilarityLoss"}


def _generator():
    spec = importlib.util.spec_from_file_location("make_torchext_surface",
                                                  os.path.join(GOLDEN, "make_torchext_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _recorded():
    with open(os.path.join(GOLDEN, "torchext_surface.json")) as f:
        return json.load(f)


def _submodules():
    return sorted(m.name for m in pkgutil.iter_modules([TORCHEXT]))


def test_functions_surface_is_the_recorded_one():
    recorded, now = _recorded(), _generator().describe()
    assert len(recorded) == 65
    assert sorted(now) == sorted(recorded)
    for name in recorded:
        assert now[name] == recorded[name], name


def test_torchext_exports_the_recorded_names_the_module_classes_and_its_submodules():
    from connecting_the_dots_amd import torchext as te
    public = {n for n in vars(te) if not n.startswith("_")}
    submodules = {n for n in public if isinstance(getattr(te, n), types.ModuleType)}
    assert submodules <= set(_submodules())
    assert not set(_submodules()) & (set(_recorded()) | MODULE_CLASSES)     # a module named as an op would hide behind it
    assert all(getattr(te, n).__name__ == "connecting_the_dots_amd.torchext." + n for n in submodules)
    assert public - submodules == set(_recorded()) | MODULE_CLASSES
    from connecting_the_dots_amd.torchext import functions
    assert sorted(functions.__all__) == sorted(_recorded())


def test_every_torchext_module_imports_in_a_fresh_interpreter():
    code = ("import importlib, sys\n"
            "for name in sys.argv[1:]:\n"
            "    importlib.import_module('connecting_the_dots_amd.torchext.' + name)\n")
    r = subprocess.run([sys.executable, "-c", code] + _submodules()[::-1], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _imports_of(path):
    """(names of the sibling modules `path` imports at module level, whether a package-relative import sits inside a
    function or class)"""
    with open(path) as f:
        tree = ast.parse(f.read())
    siblings, local = set(), False
    for node in ast.walk(tree):
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            local |= any(isinstance(n, ast.ImportFrom) and n.level > 0 for n in ast.walk(node))
    for node in tree.body:
        if isinstance(node, ast.ImportFrom) and node.level == 1:
            siblings |= {node.module} if node.module else {a.name for a in node.names}
    return siblings, local


def test_torchext_modules_are_layered_without_cycles_or_function_local_imports():
    graph = {}
    for name in _submodules():
        graph[name], local = _imports_of(os.path.join(TORCHEXT, name + ".py"))
        assert not local, "%s imports inside a function" % name
        assert graph[name] <= set(graph) | set(_submodules()), name
    depth = {}

    def layer(name, path=()):
        assert name not in path, "import cycle: %s" % " -> ".join(path + (name,))
        if name not in depth:
            depth[name] = 1 + max([layer(d, path + (name,)) for d in graph[name]], default=-1)
        return depth[name]

    for name in graph:
        layer(name)
    # a family module imports `_common` and the families below it; only `functions` (and `modules` through it) sees all
    for name, deps in graph.items():
        if name not in ("functions", "modules"):
            assert "functions" not in deps and "modules" not in deps, name
