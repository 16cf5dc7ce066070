"""The model of the index audit (tests/audit_model.py) against expectations written by hand for every case of the catalogue and
against a literal restatement of the reference's `assert_validity`, and what of ah_index_audit / ah_forest_view_audit needs no
device: the symbols and the argument checks.  The device is held against the model in tests/test_gpu_index_audit.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import audit_model as M
from arroy_amd import _lib

NONE = 0xFFFFFFFF
IDS = list(range(200))
INVALID = 5


def expect(report, valid, first_node=None, **counts):
    """exactly the given classes are non-zero, with the given counts and first offenders"""
    assert report["valid"] == valid
    for cls in M.CLASSES:
        assert report[cls] == counts.get(cls, 0), (cls, report[cls])
    for cls in M.CLASSES:
        assert report["first_node"][cls] == (first_node or {}).get(cls), (cls, report["first_node"])
    assert valid == int(not counts)


def stats(report):
    return [tuple(t[k] for k in ("root", "depth", "split_nodes", "dummy_normals", "descendants", "items")) for t in report["tree_stats"]]


@pytest.fixture(scope="module")
def cases():
    return M.catalogue(IDS)


def test_the_valid_forest(cases):
    r = cases["valid"].model(IDS, trees=True)
    expect(r, 1)
    assert (r["n_items"], r["n_trees"], r["nodes_in_use"], r["nodes_reached"]) == (200, 4, 20, 20)
    # a root that is one Descendants node; lists of 0, 1, 63, 64, 65 and 7 ids in a chain; `normal: None` over an empty
    # Descendants node; a list of 130 ids
    assert stats(r) == [(0, 1, 0, 0, 1, 200), (11, 6, 5, 0, 6, 200), (16, 3, 2, 1, 3, 200), (19, 2, 1, 0, 2, 200)]
    assert sorted(int(n) for n in cases["valid"].nodes["count"][cases["valid"].nodes["kind"] == 1])[-3:] == [100, 130, 200]
    assert {0, 1, 63, 64, 65} <= set(int(n) for n in cases["valid"].nodes["count"])
    assert r["first_missing_tree"] is None and r["first_missing_id"] is None and r["first_duplicate_tree"] is None
    assert M.plain_stats(r) == M.store_stats(cases["valid"].store())


def test_missing_and_duplicate(cases):
    r = cases["missing"].model(IDS)
    expect(r, 0, missing=1, first_node={"missing": 13})
    assert (r["first_missing_tree"], r["first_missing_id"]) == (1, 100)
    r = cases["duplicate"].model(IDS)
    expect(r, 0, duplicate=1, first_node={"duplicate": 2})
    assert (r["first_duplicate_tree"], r["first_duplicate_id"]) == (0, 100)
    expect(cases["duplicate_across_trees"].model(IDS), 1)


def test_foreign_ids():
    r = M.foreign_cases(IDS, [200, NONE]).model(IDS)
    expect(r, 0, foreign=2, first_node={"foreign": 1})
    sparse = [7 * i + 3 for i in range(199)] + [NONE]
    r = M.foreign_cases(sparse, [4, 11, NONE - 1]).model(sparse)  # ids in gaps of the sparse dataset
    expect(r, 0, foreign=3, first_node={"foreign": 0})
    expect(M.foreign_cases(sparse, []).model(sparse), 1)  # 0xFFFFFFFF where it is stored is an id like any other
    r = M.foreign_cases(sparse[:-1], [NONE]).model(sparse[:-1])  # ... and foreign where it is not
    expect(r, 0, foreign=1, first_node={"foreign": 1})


def test_unsorted_lists(cases):
    r = cases["unsorted"].model(IDS)
    # the list with the equal pair holds id 9 twice: a duplicate of its tree as well
    expect(r, 0, unsorted=3, duplicate=1, first_node={"unsorted": 0, "duplicate": 5})
    assert (r["first_duplicate_tree"], r["first_duplicate_id"]) == (1, 9)
    nd, desc = cases["unsorted"].nodes, cases["unsorted"].desc
    assert desc[63] > desc[64] and desc[int(nd["offset"][6])] > desc[int(nd["offset"][6]) + 1]


def test_floating_and_zero_trees(cases):
    r = cases["floating"].model(IDS)
    expect(r, 0, floating=3, first_node={"floating": 11})
    assert (r["nodes_in_use"], r["nodes_reached"]) == (14, 11)
    r = cases["zero_trees"].model(IDS, trees=True)
    expect(r, 1)
    assert r["tree_stats"] == [] and r["nodes_in_use"] == 0
    r = cases["zero_trees_with_nodes"].model(IDS)
    expect(r, 0, floating=4, first_node={"floating": 0})  # (no tree: nothing can be missing)


def test_the_deep_chain(cases):
    r = cases["deep_chain"].model(IDS, trees=True)
    expect(r, 1)
    assert stats(r)[0] == (78, 40, 39, 0, 40, 200)


def test_broken_structures():
    b = M.broken(IDS)
    want = {
        "two_parents": dict(linked_twice=1, floating=1, first_node={"linked_twice": 2, "floating": 10}),
        "root_is_a_child": dict(linked_twice=1, floating=3, first_node={"linked_twice": 6, "floating": 10}),
        "root_named_twice": dict(linked_twice=1, floating=7, first_node={"linked_twice": 6, "floating": 7}),
        "self_loop": dict(linked_twice=1, floating=1, first_node={"linked_twice": 5, "floating": 3}),
        "cycle_through_an_ancestor": dict(linked_twice=1, floating=1, first_node={"linked_twice": 13, "floating": 8}),
        "child_out_of_range": dict(bad_link=2, floating=2, first_node={"bad_link": 2, "floating": 1}),
        "root_out_of_range": dict(bad_root=1, floating=7, first_node={"bad_root": 0, "floating": 0}),
        "bad_kind": dict(bad_link=2, first_node={"bad_link": 5}),
        "bad_kind_root": dict(bad_root=1, floating=6, first_node={"bad_root": 1, "floating": 7}),
        "list_beyond_the_blob": dict(bad_list=2, first_node={"bad_list": 4}),
        "normal_beyond_the_blob": dict(bad_normal=2, first_node={"bad_normal": 6}),
    }
    assert sorted(want) == sorted(b)
    for name, w in want.items():
        r = M.structure_part(b[name].model(IDS))
        assert r["valid"] == 0, name
        for cls in M.STRUCTURE:
            assert r[cls] == w.get(cls, 0), (name, cls, r[cls])
            assert r["first_node"][cls] == w["first_node"].get(cls), (name, cls, r["first_node"])
    assert M.structure_part(b["bad_kind"].model(IDS))["nodes_in_use"] == 12  # (a free slot and an unknown kind are not in use)


def test_the_model_agrees_with_the_reference_where_the_reference_can_speak(cases):
    """`assert_validity` (src/reader.rs:509-589): its lists are bitmaps, so neither order nor a repetition inside one list
    exists for it, ids are not checked against anything but the item set, and it does not return from a cycle."""
    for name, c in cases.items():
        if name == "unsorted":
            continue
        assert bool(c.model(IDS)["valid"]) == M.reference_valid(c.nodes, c.roots, c.desc, IDS), name
    assert not M.reference_valid(*(lambda c: (c.nodes, c.roots, c.desc))(M.foreign_cases(IDS, [200, NONE])), IDS)
    for name, c in M.broken(IDS).items():
        if name in ("self_loop", "cycle_through_an_ancestor", "list_beyond_the_blob", "normal_beyond_the_blob"):
            continue  # (no return there; a list or a normal cannot lie outside a blob there)
        assert not c.model(IDS)["valid"] and not M.reference_valid(c.nodes, c.roots, c.desc, IDS), name
    # the contracts: a delete the dataset did not follow, an update the index did not follow
    c = M.catalogue(IDS)["valid"]
    assert c.model(IDS + [500])["missing"] == 4 and not M.reference_valid(c.nodes, c.roots, c.desc, IDS + [500])
    assert c.model(IDS[:-2])["foreign"] == 8 and not M.reference_valid(c.nodes, c.roots, c.desc, IDS[:-2])


def test_random_forests_model_against_the_reference():
    seen = set()
    stored = IDS
    for seed in range(50):
        c = M.random_case(seed, stored)
        r = c.model(stored)
        lists_are_sets = r["unsorted"] == 0
        if lists_are_sets:
            assert bool(r["valid"]) == M.reference_valid(c.nodes, c.roots, c.desc, stored), seed
        seen.update(k for k in M.CLASSES if r[k])
    assert {"unsorted", "foreign", "duplicate", "missing"} <= seen


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------

def test_the_header_declares_both_symbols_and_the_library_exports_them():
    src = open(os.path.join(ROOT, "include", "arroy_hip.h")).read()
    declared = set(re.findall(r"^AH_API [^;(]*?\b(ah_[a-z_0-9]+)\s*\(", src, re.M))
    assert {"ah_index_audit", "ah_forest_view_audit"} <= declared
    L = C.CDLL(_lib.build())
    assert hasattr(L, "ah_index_audit") and hasattr(L, "ah_forest_view_audit")
    assert "ah_index_audit" in _lib.SIGNATURES and "ah_forest_view_audit" in _lib.SIGNATURES
    # the report as the header lays it out
    assert C.sizeof(_lib.AhTreeStats) == 32 and C.sizeof(_lib.AhIndexAuditReport) == 4 * 8 + 10 * 8 + 10 * 4 + 6 * 4
    assert re.search(r"AH_AUDIT_BAD_ROOT, AH_AUDIT_BAD_LINK, AH_AUDIT_LINKED_TWICE, AH_AUDIT_FLOATING, AH_AUDIT_BAD_NORMAL,\s*"
                     r"AH_AUDIT_BAD_LIST, AH_AUDIT_UNSORTED, AH_AUDIT_FOREIGN, AH_AUDIT_DUPLICATE, AH_AUDIT_MISSING, AH_AUDIT_CLASSES", src)
    assert [c.upper() for c in _lib.AUDIT_CLASSES] == ["BAD_ROOT", "BAD_LINK", "LINKED_TWICE", "FLOATING", "BAD_NORMAL", "BAD_LIST",
                                                       "UNSORTED", "FOREIGN", "DUPLICATE", "MISSING"]


def test_null_arguments_are_refused_and_the_report_is_untouched():
    L = _lib.lib()
    rep = _lib.AhIndexAuditReport()
    C.memset(C.byref(rep), 0xAB, C.sizeof(rep))
    before = bytes(rep)
    assert L.ah_index_audit(None, C.byref(rep), None) == INVALID and b"index is NULL" in L.ah_last_error()
    assert L.ah_index_audit(None, None, None) == INVALID and b"out is NULL" in L.ah_last_error()
    view = _lib.AhForestView()
    assert L.ah_forest_view_audit(None, None, C.byref(rep), None) == INVALID and b"view is NULL" in L.ah_last_error()
    assert L.ah_forest_view_audit(None, C.byref(view), None, None) == INVALID and b"out is NULL" in L.ah_last_error()
    assert L.ah_forest_view_audit(None, C.byref(view), C.byref(rep), None) == INVALID and b"dataset is NULL" in L.ah_last_error()
    assert bytes(rep) == before


def test_the_tunable_exists_with_its_default():
    assert _lib.tuning_get("AH_AUDIT_COVER_MB") == (64, 64)
