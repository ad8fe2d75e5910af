"""Generate tests/golden/torchext_surface.json: the public surface of `connecting_the_dots_amd.torchext.functions`.

    python tests/golden/make_torchext_surface.py

For every public name: its kind (function | class | int), `str(inspect.signature(...))` (for a class also of `forward`
and `backward` where it has them), the SHA-256 of its `__doc__` as it stands after import (the `__doc__ += _RULE` lines
have run) and, for a constant, its value.  Needs neither a GPU nor the built library.  tests/test_torchext_surface.py
asserts that `describe()` still returns what the file holds; regenerate it only when the surface is meant to change.
"""
import hashlib
import inspect
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torchext_surface.json")


def public_names(mod):
    """`__all__` where the module has one; otherwise what `import *` takes, without the modules it imported itself"""
    if hasattr(mod, "__all__"):
        return sorted(mod.__all__)
    return sorted(n for n, v in vars(mod).items() if not n.startswith("_") and not isinstance(v, types.ModuleType))


def _doc_hash(obj):
    return hashlib.sha256((obj.__doc__ or "").encode("utf-8")).hexdigest()


def _describe_one(obj):
    if isinstance(obj, bool) or not isinstance(obj, (int, type, types.FunctionType)):
        raise TypeError("unexpected kind of public name: %r" % (obj,))
    if isinstance(obj, int):
        return {"kind": "int", "value": obj}
    if isinstance(obj, type):
        d = {"kind": "class", "doc_sha256": _doc_hash(obj)}
        for m in ("__init__", "forward", "backward"):
            if m in vars(obj):
                d[m] = str(inspect.signature(getattr(vars(obj)[m], "__func__", vars(obj)[m])))
        return d
    return {"kind": "function", "signature": str(inspect.signature(obj)), "doc_sha256": _doc_hash(obj)}


def describe():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from connecting_the_dots_amd.torchext import functions
    return {name: _describe_one(getattr(functions, name)) for name in public_names(functions)}


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(describe(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d names" % (OUT, len(describe())))
