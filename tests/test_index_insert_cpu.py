"""ah_index_insert_items / ah_index_graft / ah_index_export without a GPU: the symbols against the header and the export map,
and what the calls refuse before they look at an index (tests/test_gpu_index_insert.py runs the kernels)."""
import ctypes as C
import os
import re

import numpy as np

from arroy_amd import _lib
from conftest import ROOT

NEW = ("ah_index_insert_items", "ah_index_graft", "ah_index_export_info", "ah_index_export")
INVALID = 5


def test_new_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "arroy_hip.h")).read()
    declared = set(re.findall(r"^AH_API [^;(]*?\b(ah_[a-z_0-9]+)\s*\(", header, re.M))
    exports = open(os.path.join(ROOT, "arroy_amd", "csrc", "exports.map")).read()
    assert "global: ah_*;" in exports  # every ah_ symbol of the C ABI is exported by the pattern
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert "#define AH_NEW_ROOT 0xFFFFFFFFu" in header and _lib.NEW_ROOT == 0xFFFFFFFF
    assert L.ah_abi_version() == 7
    assert C.sizeof(_lib.AhIndexInfo) == 40


def test_refusals_that_need_no_index():
    L = _lib.lib()
    out = C.c_void_p()
    ids = np.array([1, 2, 5], dtype=np.uint32)
    seeds = np.array([1, 2], dtype=np.uint64)

    def insert(arr, n, delta):
        st = L.ah_index_insert_items(None, None if arr is None else arr.ctypes.data_as(C.c_void_p), n, seeds.ctypes.data_as(C.c_void_p),
                                     delta)
        return st, L.ah_last_error().decode()

    st, msg = insert(ids, 3, C.byref(out))
    assert st == INVALID and "index is NULL" in msg and not out
    st, msg = insert(ids, 3, None)
    assert st == INVALID and "out_delta is NULL" in msg
    st, msg = insert(None, 3, C.byref(out))
    assert st == INVALID and "sorted_ids is NULL" in msg
    st, msg = insert(np.array([1, 5, 2], dtype=np.uint32), 3, C.byref(out))
    assert st == INVALID and "not strictly ascending" in msg and "position 2" in msg
    assert L.ah_index_graft(None, None, None, None, None) == INVALID and b"index is NULL" in L.ah_last_error()
    assert L.ah_index_export_info(None, C.byref(_lib.AhIndexInfo())) == INVALID
    assert L.ah_index_export(None, None, None, None, None, None) == INVALID
