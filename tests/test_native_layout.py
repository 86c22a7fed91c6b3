"""CPU checks of the layout rules of gans/models/ops/native/ (DESIGN.md section 27): explicit imports and literal
__all__ lists, the public surface of the package, switches never imported by name, no import-order dependence.
Needs the built library (the package imports dgv2_native), no GPU."""
import ast
import importlib
import os
import pkgutil
import re
import subprocess
import sys

import pytest

from conftest import GOLDEN, PKG, ROOT

NATIVE_DIR = os.path.join(PKG, "gans", "models", "ops", "native")
NATIVE = "gans.models.ops.native"
SUBMODULES = sorted(m.name for m in pkgutil.iter_modules([NATIVE_DIR]))
SWITCH_NAME = re.compile(r"_[A-Z][A-Z0-9_]*")


def _tree(name):
    with open(os.path.join(NATIVE_DIR, name + ".py")) as f:
        return ast.parse(f.read())


def _submodule(name):
    return importlib.import_module(f"{NATIVE}.{name}")


def test_submodules_found():
    assert {"act_resample", "conv", "modgemm", "modlayer", "fp8"} <= set(SUBMODULES) and "misc" not in SUBMODULES


@pytest.mark.parametrize("name", SUBMODULES)
def test_no_star_import_and_literal_all(name):
    """(a) only __init__.py star-imports; every submodule's __all__ is a literal list of strings."""
    tree = _tree(name)
    stars = [n.lineno for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and any(a.name == "*" for a in n.names)]
    assert not stars, f"{name}.py: star import at line(s) {stars}"
    local = [n.lineno for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom)) and n.col_offset > 0]
    assert not local, f"{name}.py: import below module level at line(s) {local}"
    alls = [n for n in tree.body if isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "__all__" for t in n.targets)]
    assert len(alls) == 1, f"{name}.py: expected exactly one module-level __all__"
    val = alls[0].value
    assert isinstance(val, ast.List) and all(isinstance(e, ast.Constant) and isinstance(e.value, str) for e in val.elts), \
        f"{name}.py: __all__ must be a literal list of strings"
    mod = _submodule(name)
    missing = [n for n in mod.__all__ if not hasattr(mod, n)]
    assert not missing, f"{name}.__all__ names what the module does not have: {missing}"


def test_init_has_no_computed_all():
    tree = _tree("__init__")
    assert not [n for n in ast.walk(tree) if isinstance(n, ast.Name) and n.id == "__all__"]


def _defined_in(mod, name):
    """Whether `mod` itself defines `name` (a def / class / assignment of its own file, not an import)."""
    for node in _tree(mod.__name__.rsplit(".", 1)[1]).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name == name:
            return True
        if isinstance(node, (ast.Assign, ast.If)):
            if any(isinstance(n, ast.Name) and n.id == name and isinstance(n.ctx, ast.Store) for n in ast.walk(node)):
                return True
    return False


def test_public_surface():
    """(b) every name the rest of the tree used as native.<name> resolves, and is the object its defining submodule holds."""
    native = importlib.import_module(NATIVE)
    with open(os.path.join(GOLDEN, "native_public_names.txt")) as f:
        names = f.read().split()
    assert len(names) >= 115     # (116 before ABI 59 retired _conv_taps with the tap-list entries)
    mods = {m: _submodule(m) for m in SUBMODULES}
    for name in names:
        assert hasattr(native, name), f"native.{name} no longer resolves"
        obj = getattr(native, name)
        if name in mods:
            assert obj is mods[name]
            continue
        if name == "N":
            import dgv2_native
            assert obj is dgv2_native
            continue
        owners = [m for m, mod in mods.items() if _defined_in(mod, name)]
        assert len(owners) == 1, f"native.{name}: defined in {owners}, expected exactly one submodule"
        assert obj is getattr(mods[owners[0]], name), f"native.{name} is not {owners[0]}.{name}"


def test_switches_are_never_imported_by_name():
    """(c) a submodule global named like a switch / module constant (_UPPER_CASE; bool, int, tuple or dict) is bound in
    no other submodule: the others read <module>.<FLAG>, so that flipping the flag at run time reaches every reader."""
    mods = {m: _submodule(m) for m in SUBMODULES}
    for m, mod in mods.items():
        for name, val in vars(mod).items():
            if not SWITCH_NAME.fullmatch(name) or not isinstance(val, (bool, int, tuple, dict)):
                continue
            others = [o for o, omod in mods.items() if o != m and name in vars(omod)]
            assert not others, f"{name} of {m} is also bound in {others}"


@pytest.mark.parametrize("name", SUBMODULES)
def test_each_submodule_imports_first(name):
    """(d) importing any one submodule first, in a fresh interpreter, succeeds (no order-dependent cycle)."""
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}]; import importlib; "
            f"importlib.import_module('{NATIVE}.{name}'); import {NATIVE} as n; assert n.{name}")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
