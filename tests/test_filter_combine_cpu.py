"""ah_filter_combine / ah_filter_create_bitmap / ah_filter_export without a GPU: the symbols against the header and the ctypes
table, the refusals that are judged before a device is touched, and the rules by which k_leaf_kept_combine derives a leaf's
count from its operands' counts, restated in numpy (`derive`) and checked exhaustively against set arithmetic on small leaves.
tests/test_gpu_filter_combine.py imports `derive` and holds ah_filter_combine_stats of real calls against it."""
import ctypes as C
import itertools
import os
import re

import numpy as np

from conftest import ROOT

AND, OR, ANDNOT, NOT = 0, 1, 2, 3
OPS = (AND, OR, ANDNOT, NOT)
COMBINE_MAX = 64
NEW_SYMBOLS = ("ah_filter_combine", "ah_filter_create_bitmap", "ah_filter_export")
WALK = "walk"


def derive(op, c, ks):
    """What a leaf of `c` ids keeps under the expression, from the counts `ks` its operands keep of it — or WALK where the
    counts do not settle it and the leaf's ids have to be tested against the new bitmap (DESIGN.md §4 "Combined filters")."""
    ks = [int(k) for k in ks]
    c = int(c)
    if c == 0:
        return 0
    if op == NOT:
        return c - ks[0]
    if op == AND:
        if any(k == 0 for k in ks):
            return 0
        return min(ks) if sum(k < c for k in ks) <= 1 else WALK
    if op == OR:
        if any(k == c for k in ks):
            return c
        return max(ks) if sum(k > 0 for k in ks) <= 1 else WALK
    if op == ANDNOT:
        if ks[0] == 0 or any(k == c for k in ks[1:]):
            return 0
        return ks[0] if all(k == 0 for k in ks[1:]) else WALK
    raise ValueError(op)


def evaluate(op, sets, universe):
    """The expression over Python sets: the yardstick of `derive`."""
    if op == AND:
        return set.intersection(*sets)
    if op == OR:
        return set.union(*sets)
    if op == ANDNOT:
        return sets[0] - set.union(set(), *sets[1:])
    return universe - sets[0]


def test_new_symbols_are_declared_exported_and_bound():
    from arroy_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "arroy_hip.h")).read()
    declared = set(re.findall(r"^AH_API [^;(]*?\b(ah_[a-z_0-9]+)\s*\(", header, re.M))
    assert "global: ah_*;" in open(os.path.join(ROOT, "arroy_amd", "csrc", "exports.map")).read()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.ah_abi_version() == 7
    assert "AH_FILTER_AND = 0, AH_FILTER_OR = 1, AH_FILTER_ANDNOT = 2, AH_FILTER_NOT = 3" in header
    assert (_lib.FILTER_AND, _lib.FILTER_OR, _lib.FILTER_ANDNOT, _lib.FILTER_NOT) == OPS
    assert "#define AH_FILTER_COMBINE_MAX 64" in header and _lib.FILTER_COMBINE_MAX == COMBINE_MAX
    assert C.sizeof(_lib.AhFilterCombineStats) == 4 * 8
    assert C.sizeof(_lib.AhFilterStats) == 8 * 8  # existing callers pass the eight-field struct: it has not grown
    assert _lib.tuning_get("AH_FILTER_COMBINE_SHORTCUT") == (1, 1)


def test_refusals_that_need_no_device():
    from arroy_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    st = _lib.AhFilterCombineStats()
    two = (C.c_void_p * 2)(None, None)
    many = (C.c_void_p * (COMBINE_MAX + 1))()

    def refused(status, *words):
        assert status == 5, status  # AH_ERR_INVALID_ARGUMENT
        for word in words:
            assert word in L.ah_last_error().decode(), L.ah_last_error()
        assert not h.value

    refused(L.ah_filter_combine(AND, two, 2, None, C.byref(st)), "out is NULL")
    refused(L.ah_filter_combine(AND, two, 0, C.byref(h), None), "n = 0")
    refused(L.ah_filter_combine(OR, many, COMBINE_MAX + 1, C.byref(h), None), "n = 65", "64")
    refused(L.ah_filter_combine(NOT, two, 2, C.byref(h), None), "AH_FILTER_NOT", "exactly one", "n = 2")
    for op in (4, -1, 1000):
        refused(L.ah_filter_combine(op, two, 1, C.byref(h), None), f"unknown op {op}")
    refused(L.ah_filter_combine(AND, C.POINTER(C.c_void_p)(), 2, C.byref(h), None), "operands is NULL")
    for op in (AND, OR, ANDNOT):
        refused(L.ah_filter_combine(op, two, 2, C.byref(h), None), "operands[0] is NULL")
    refused(L.ah_filter_combine(NOT, two, 1, C.byref(h), C.byref(st)), "operands[0] is NULL")
    # ah_filter_create_bitmap: a NULL out, NULL words with a length, a NULL index (n_bits == 0 needs no words)
    words = np.array([5, 0], np.uint64)
    p = words.ctypes.data_as(C.c_void_p)
    refused(L.ah_filter_create_bitmap(None, p, 100, None), "out is NULL")
    refused(L.ah_filter_create_bitmap(None, None, 100, C.byref(h)), "words is NULL")
    refused(L.ah_filter_create_bitmap(None, p, 100, C.byref(h)), "index is NULL")
    refused(L.ah_filter_create_bitmap(None, None, 0, C.byref(h)), "index is NULL")
    refused(L.ah_filter_export(None, None, None, None), "filter is NULL")


def test_derive_equals_set_arithmetic_on_every_small_leaf():
    """Every leaf of up to 4 ids, every choice of up to three operands among its subsets, every op: where `derive` gives a
    count it is the count, and it gives one in exactly the cases the rules name (at most one operand that keeps a part)."""
    derived = walked = 0
    for c in range(0, 5):
        universe = set(range(c))
        subsets = [set(s) for r in range(c + 1) for s in itertools.combinations(range(c), r)]
        for n in (1, 2, 3):
            for sets in itertools.product(subsets, repeat=n):
                ks = [len(s) for s in sets]
                for op in OPS:
                    if op == NOT and n != 1:
                        continue
                    got = derive(op, c, ks)
                    want = len(evaluate(op, list(sets), universe))
                    if got == WALK:
                        walked += 1
                        assert c > 0
                    else:
                        derived += 1
                        assert got == want, (op, c, sets, got, want)
                    if n == 1:
                        assert got != WALK and (op == NOT or got == ks[0])  # a copy; NOT never walks
    assert derived > 1000 and walked > 1000
    # the walks are exactly the leaves where two or more operands keep a part that can change the result
    assert derive(AND, 4, [2, 3, 4]) == WALK and derive(AND, 4, [4, 3, 4]) == 3 and derive(AND, 4, [2, 0, 3]) == 0
    assert derive(OR, 4, [1, 2, 0]) == WALK and derive(OR, 4, [0, 2, 0]) == 2 and derive(OR, 4, [1, 4, 2]) == 4
    assert derive(ANDNOT, 4, [3, 1]) == WALK and derive(ANDNOT, 4, [3, 0, 0]) == 3 and derive(ANDNOT, 4, [3, 1, 4]) == 0
    assert derive(ANDNOT, 4, [0, 1, 2]) == 0 and derive(NOT, 4, [1]) == 3
