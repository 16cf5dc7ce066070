"""Every tunable is flipped by a GPU test, or this file says why not (no GPU needed).

DESIGN.md §4 promises bit-identical results under every setting of every entry of AH_TUNABLES (arroy_amd/csrc/common.h).  A
switch no test sets is a code path — often whole kernel instantiations — that is compiled, shipped, selectable and unchecked.
A GPU test "sets" a tunable when its name is a keyword argument of a call (`tuning(AH_X=...)`, `dict(AH_X=...)`,
`dict(os.environ, AH_X=...)`) or a string constant of its own (a dict key, an entry of a list of switch names) in some
tests/test_gpu_*.py; comments and prose in docstrings do not count (the files are parsed, not searched).  A new tunable fails
this test until someone flips it against a reference or states here why its value cannot change a result."""
import ast
import glob
import os
import re

from conftest import ROOT

# switches that select no code path whose result can differ
EXEMPT = {
    "AH_TIMING": "prints timings on stderr; no kernel or schedule reads it",
    "AH_RERANK_TIMING": "accounts wall time by phase in ah_dataset_rerank_stats; the submission is the same",
    "AH_SEARCH_MULTI_TRACE": "prints where the blocks of query 0 spent their time; the kernel's extra stores go to trace words only",
    "AH_STAGE_THREADS": "read once, when the process-wide staging pool starts: cannot be flipped in-process after the first upload",
    "AH_CACHE_KEEP_IDLE": "keeps the allocators' idle memory past the last dataset; no kernel or schedule reads it",
}


def tunables():
    hdr = open(os.path.join(ROOT, "arroy_amd", "csrc", "common.h")).read()
    names = re.findall(r'X\(\w+, "(AH_[A-Z0-9_]+)"', hdr)
    assert len(names) >= 30 and len(set(names)) == len(names)
    return names


def names_set_by(path):
    """The AH_* names a test file sets: keyword arguments of calls and string constants that are exactly such a name."""
    found = set()
    for node in ast.walk(ast.parse(open(path).read(), filename=path)):
        if isinstance(node, ast.Call):
            found.update(kw.arg for kw in node.keywords if kw.arg and kw.arg.startswith("AH_"))
        elif isinstance(node, ast.Constant) and isinstance(node.value, str) and re.fullmatch(r"AH_[A-Z0-9_]+", node.value):
            found.add(node.value)
    return found


def set_by_gpu_tests():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))
    assert len(files) >= 25
    by_name = {}
    for path in files:
        for name in names_set_by(path):
            by_name.setdefault(name, []).append(os.path.basename(path))
    return by_name


def test_every_tunable_is_flipped_by_a_gpu_test_or_exempt_with_a_reason():
    used = set_by_gpu_tests()
    missing = [n for n in tunables() if n not in used and n not in EXEMPT]
    assert not missing, f"tunables no tests/test_gpu_*.py sets and EXEMPT does not explain: {missing}"


def test_exemptions_are_tunables_nobody_sets_and_carry_a_reason():
    names, used = set(tunables()), set_by_gpu_tests()
    assert not [n for n in EXEMPT if n not in names], "EXEMPT names something that is not a tunable"
    assert not [n for n in EXEMPT if n in used], "EXEMPT names a tunable that a GPU test sets: drop the exemption"
    assert all(len(reason) > 20 for reason in EXEMPT.values())


def test_the_parser_sees_keywords_and_keys_but_not_comments_or_prose(tmp_path):
    src = tmp_path / "sample.py"
    src.write_text('"""prose: AH_IN_DOCSTRING=1 and \'AH_QUOTED_IN_DOCSTRING\'."""\n'
                   "# tuning(AH_IN_COMMENT=1)\n"
                   "with tuning(AH_KEYWORD=0, **{'AH_DICT_KEY': 1}):\n    pass\n"
                   "env = dict(os.environ, AH_ENV_KEYWORD='1')\nKNOBS = ['AH_LIST_ENTRY']\nenv['AH_SUBSCRIPT'] = '1'\n"
                   "SCRIPT = 'tuning(AH_INSIDE_A_SCRIPT=1)'\n")
    assert names_set_by(str(src)) == {"AH_KEYWORD", "AH_DICT_KEY", "AH_ENV_KEYWORD", "AH_LIST_ENTRY", "AH_SUBSCRIPT"}
