"""CPU-side checks of the dataset update calls: declared in the header, exported by the library, bound in SIGNATURES, and
refused with a status code (never an exception) before any device is touched."""
import ctypes
import os
import re

from conftest import ROOT

UPDATE_CALLS = ["ah_dataset_update_vectors", "ah_dataset_update_records", "ah_group_update_vectors", "ah_group_update_records",
                "ah_debug_update_paths"]


def test_update_calls_are_declared_exported_and_bound():
    from arroy_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "arroy_hip.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in UPDATE_CALLS:
        assert re.search(r"^AH_API int %s\(" % name, hdr, re.M), name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.lib().ah_abi_version() == 7  # additions only


def test_update_calls_refuse_null_handles():
    from arroy_amd import _lib
    L = _lib.lib()
    assert L.ah_dataset_update_vectors(None, None, 0, None, None, 0) == 5
    assert L.ah_dataset_update_records(None, None, 0, None, None, 0, 0) == 5
    assert L.ah_group_update_vectors(None, None, 0, None, None, 0) == 5
    assert L.ah_group_update_records(None, None, 0, None, None, 0, 0) == 5
    assert L.ah_debug_update_paths(None, None, None, None) == 5
    assert b"NULL" in L.ah_last_error()
