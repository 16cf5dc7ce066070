"""Every exported entry point is reached by a GPU test, or this file says why not (no GPU needed).

include/arroy_hip.h is the product: every `AH_API` function is compiled, exported and callable by the Rust side.  An entry point
no GPU test reaches is device code nothing compares with the oracle — `ah_margins` was the only caller of a whole branch of both
single-node margin kernels and had never run.  This is the rule of test_tunable_coverage_cpu.py for the C ABI.

A tests/test_gpu_*.py "reaches" a symbol when
  - it names the symbol in code: an attribute (`lib().ah_margins`), a bare name, or a string constant that is exactly the
    symbol (`getattr(L, "ah_margins")`); or
  - it reads an attribute, or calls a bare name, that is spelled like a function, method or property of arroy_amd/*.py whose
    body names the symbol — followed transitively through the package, by NAME: `ds.margins(...)` reaches whatever any
    `def margins` of the package reaches.  `__init__` is spelled like its class, `__len__` like `len`, the other special
    methods like nothing (Filter's operators call `combine_filters`, `__del__` calls `close`: the tests spell those).
The files are parsed, not searched: comments and docstrings do not count.  Resolution by name is generous — `close` is every
class's `close` — so this test can miss an unreached entry point that shares a wrapper's name with a reached one; it cannot
report a reached one as missing.  A new entry point fails this test until a GPU test calls it against a reference, or it is
listed below with the reason."""
import ast
import glob
import os
import re

from conftest import ROOT

# entry points that touch no device: reached by a host test (tests/test_*.py that is no test_gpu_*.py) instead
HOST_ONLY = {
    "ah_abi_version": "returns the constant AH_ABI_VERSION of the header; no device, no dataset, nothing to compare on a GPU",
}

# entry points no test has to call (none so far)
EXEMPT = {}

DUNDER_SPELLING = {"__len__": "len"}  # `__init__` -> the class name (below)


def abi_functions():
    hdr = open(os.path.join(ROOT, "include", "arroy_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)  # (a comment may quote a declaration)
    names = re.findall(r"\bAH_API\b[^;{()]*?\b(ah_\w+)\s*\(", hdr)
    assert len(names) >= 120 and len(set(names)) == len(names)
    return names


def _strip_docstrings(tree):
    for node in ast.walk(tree):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body:
            first = node.body[0]
            if isinstance(first, ast.Expr) and isinstance(first.value, ast.Constant) and isinstance(first.value.value, str):
                node.body = node.body[1:] or [ast.Pass()]
    return tree


def names_used(node):
    """What code under `node` calls or reads by name: every attribute name, every bare name that is called, and every `ah_*`
    bare name or string constant.  (A bare name that is only assigned or passed on is a local: `margins = ds.split_sides(...)`
    must not reach a method called `margins`.)"""
    found = set()
    for n in ast.walk(node):
        if isinstance(n, ast.Attribute):
            found.add(n.attr)
        elif isinstance(n, ast.Call) and isinstance(n.func, ast.Name):
            found.add(n.func.id)
        elif isinstance(n, ast.Name) and n.id.startswith("ah_"):
            found.add(n.id)
        elif isinstance(n, ast.Constant) and isinstance(n.value, str) and re.fullmatch(r"ah_\w+", n.value):
            found.add(n.value)
    return found


def names_used_by_file(path):
    return names_used(_strip_docstrings(ast.parse(open(path).read(), filename=path)))


def package_definitions(paths):
    """spelling -> the identifiers the bodies of every def of that spelling use (methods, properties, functions, nested defs
    counted with the def that encloses them)."""
    defs = {}

    def add(spelling, node):
        defs.setdefault(spelling, set()).update(names_used(node))

    for path in paths:
        tree = _strip_docstrings(ast.parse(open(path).read(), filename=path))
        for top in tree.body:
            if isinstance(top, (ast.FunctionDef, ast.AsyncFunctionDef)):
                add(top.name, top)
            elif isinstance(top, ast.ClassDef):
                for item in top.body:
                    if isinstance(item, (ast.FunctionDef, ast.AsyncFunctionDef)):
                        spelling = top.name if item.name == "__init__" else DUNDER_SPELLING.get(item.name, item.name)
                        if spelling.startswith("__") and spelling.endswith("__"):
                            continue
                        add(spelling, item)
    return defs


def symbols_reached(used, defs, symbols):
    """The symbols the identifiers `used` reach: themselves, and through the package's definitions by name."""
    seen, todo, hit = set(), list(used), set()
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        if name in symbols:
            hit.add(name)
        todo.extend(defs.get(name, ()))
    return hit


def reached_by(pattern, exclude=None):
    symbols = set(abi_functions())
    defs = package_definitions(sorted(glob.glob(os.path.join(ROOT, "arroy_amd", "*.py"))))
    files = [p for p in sorted(glob.glob(os.path.join(ROOT, "tests", pattern))) if not (exclude and exclude(os.path.basename(p)))]
    by_symbol = {}
    for path in files:
        for s in symbols_reached(names_used_by_file(path), defs, symbols):
            by_symbol.setdefault(s, []).append(os.path.basename(path))
    return by_symbol, files


def test_every_entry_point_is_reached_by_a_gpu_test_or_listed_with_a_reason():
    reached, files = reached_by("test_gpu_*.py")
    assert len(files) >= 25
    missing = [s for s in abi_functions() if s not in reached and s not in HOST_ONLY and s not in EXEMPT]
    assert not missing, f"entry points no tests/test_gpu_*.py reaches and neither HOST_ONLY nor EXEMPT explains: {missing}"


def test_host_only_entry_points_are_reached_by_a_host_test():
    reached, _ = reached_by("test_*.py", exclude=lambda name: name.startswith("test_gpu_"))
    assert not [s for s in HOST_ONLY if s not in reached], "HOST_ONLY names an entry point no host test reaches"


def test_the_lists_name_entry_points_nobody_reaches_and_carry_a_reason():
    symbols, (reached, _) = set(abi_functions()), reached_by("test_gpu_*.py")
    for table in (HOST_ONLY, EXEMPT):
        assert not [s for s in table if s not in symbols], "a list names something that is not an entry point"
        assert not [s for s in table if s in reached], "a list names an entry point that a GPU test reaches: drop the entry"
        assert all(len(reason) > 20 for reason in table.values())
    assert not set(HOST_ONLY) & set(EXEMPT)


def test_the_binding_declares_exactly_the_header():
    """arroy_amd/_lib.py resolves every name of SIGNATURES at load; a declaration the binding lacks is one Python cannot reach."""
    tree = ast.parse(open(os.path.join(ROOT, "arroy_amd", "_lib.py")).read())
    table = next(n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "SIGNATURES")
    bound = {k.value for k in table.keys}
    assert bound == set(abi_functions()), sorted(bound ^ set(abi_functions()))


def test_the_parser_follows_names_through_the_package_but_not_comments_or_prose(tmp_path):
    pkg = tmp_path / "pkg.py"
    pkg.write_text('"""prose: ah_in_module_docstring()."""\n'
                   "def helper():\n    return lib().ah_via_helper()\n"
                   "def unrelated():\n    '''ah_in_docstring'''\n    # ah_in_comment\n    return lib().ah_unreached()\n"
                   "class Thing:\n"
                   "    def __init__(self):\n        lib().ah_in_init()\n"
                   "    def __len__(self):\n        return lib().ah_in_len()\n"
                   "    def __del__(self):\n        lib().ah_in_del()\n"
                   "    @property\n    def prop(self):\n        return lib().ah_in_property()\n"
                   "    def method(self):\n        def inner():\n            return helper()\n        return inner()\n"
                   "    def by_string(self):\n        return getattr(lib(), 'ah_by_string')()\n")
    symbols = {"ah_via_helper", "ah_unreached", "ah_in_init", "ah_in_len", "ah_in_del", "ah_in_property", "ah_by_string",
               "ah_in_docstring", "ah_in_comment", "ah_in_module_docstring", "ah_direct", "ah_in_test_comment", "ah_in_test_prose"}
    defs = package_definitions([str(pkg)])

    def reach(src):
        test = tmp_path / "sample.py"
        test.write_text(src)
        return symbols_reached(names_used_by_file(str(test)), defs, symbols)

    assert reach('"""ah_in_test_prose"""\n# t.method(); lib().ah_in_test_comment\nx = 1\n') == set()
    assert reach("t.method()\n") == {"ah_via_helper"}          # method -> nested def -> helper -> symbol
    assert reach("t = Thing()\n") == {"ah_in_init"}            # the class is spelled like its __init__
    assert reach("n = len(t)\n") == {"ah_in_len"}
    assert reach("v = t.prop\n") == {"ah_in_property"}         # a property is read, not called
    assert reach("t.by_string()\n") == {"ah_by_string"}
    assert reach("L.ah_direct(None)\nf = getattr(L, 'ah_unreached')\n") == {"ah_direct", "ah_unreached"}
    assert reach("SCRIPT = 't.method(); lib().ah_direct()'\ndel t\n") == set()  # code kept in a string is not parsed
