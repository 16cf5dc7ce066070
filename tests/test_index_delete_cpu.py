"""ah_index_delete_items / ah_index_suspend / ah_index_resume without a GPU: the symbols, what the calls refuse before they
look at an index, and TreeStore.apply_delta on a delta written by hand (tests/test_gpu_index_delete.py runs the kernels)."""
import ctypes as C

import numpy as np

from arroy_amd import _lib
from arroy_amd.index import TreeStore

NEW = ("ah_index_delete_items", "ah_index_delta_get", "ah_index_delta_destroy", "ah_index_suspend", "ah_index_resume")
INVALID = 5


def test_new_symbols_are_exported_and_the_abi_version_stays():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.ah_abi_version() == 7


def test_refusals_that_need_no_index():
    L = _lib.lib()
    out = C.c_void_p()
    ids = np.array([1, 2, 5], dtype=np.uint32)

    def call(index, arr, n, delta):
        st = L.ah_index_delete_items(index, None if arr is None else arr.ctypes.data_as(C.c_void_p), n, 8, delta)
        return st, L.ah_last_error().decode()

    st, msg = call(None, ids, 3, C.byref(out))
    assert st == INVALID and "index is NULL" in msg and not out
    st, msg = call(None, ids, 3, None)
    assert st == INVALID and "out_delta is NULL" in msg
    st, msg = call(None, None, 3, C.byref(out))
    assert st == INVALID and "sorted_ids is NULL" in msg
    st, msg = call(None, np.array([1, 5, 2], dtype=np.uint32), 3, C.byref(out))
    assert st == INVALID and "not strictly ascending" in msg and "position 2" in msg
    st, msg = call(None, np.array([1, 5, 5], dtype=np.uint32), 3, C.byref(out))
    assert st == INVALID and "not strictly ascending" in msg
    assert L.ah_index_delta_destroy(None) == 0
    assert L.ah_index_delta_get(None, C.byref(_lib.AhIndexDeltaView())) == INVALID
    assert L.ah_index_suspend(None) == INVALID and L.ah_index_resume(None, None) == INVALID


def test_apply_delta_on_a_hand_written_delta():
    """Store ids 10 .. 16 are the dense indices 0 .. 6 of the view.  The delta: node 12 (a leaf) lost an id, the split 13
    merged its leaves 10 and 11 away, the split 16 was replaced by its child 15 (its other child 14 emptied), so the root of
    the second tree is now 15."""
    hdr, vec = np.zeros(1, np.float32), b"\0" * 16
    s = TreeStore()
    s.nodes = {10: ("D", np.array([1, 2], np.uint32)), 11: ("D", np.array([3, 4], np.uint32)), 12: ("D", np.array([5, 6, 7], np.uint32)),
               13: ("S", 10, 11, hdr, vec), 17: ("S", 13, 12, hdr, vec),
               14: ("D", np.array([8], np.uint32)), 15: ("D", np.array([9, 10, 11], np.uint32)), 16: ("S", 14, 15, hdr, None)}
    s.roots = [16, 17]
    dense = {nid: i for i, nid in enumerate(sorted(s.nodes))}
    node_dt = np.dtype([("kind", "u1"), ("has_normal", "u1"), ("reserved", "<u2"), ("tree", "<u4"), ("left", "<u4"),
                        ("right", "<u4"), ("offset", "<u8"), ("count", "<u4"), ("depth", "<u4")], align=True)
    put = np.zeros(2, node_dt)
    put[0] = (1, 0, 0, 0, 0, 0, 0, 2, 0)   # node 12: ids desc[0:2]
    put[1] = (1, 0, 0, 0, 0, 0, 2, 3, 0)   # node 13: ids desc[2:5]
    delta = {"removed": np.array([dense[10], dense[11], dense[14], dense[16]], np.uint32),
             "put_index": np.array([dense[12], dense[13]], np.uint32), "put": put,
             "desc": np.array([5, 7, 1, 2, 4], np.uint32), "roots": np.array([dense[15], dense[17]], np.uint32)}
    s.apply_delta(delta, dense)
    assert sorted(s.nodes) == [12, 13, 15, 17] and s.roots == [15, 17]
    assert s.nodes[12][0] == "D" and s.nodes[12][1].tolist() == [5, 7] and s.nodes[12][1].dtype == np.uint32
    assert s.nodes[13][0] == "D" and s.nodes[13][1].tolist() == [1, 2, 4]
    assert s.nodes[15][1].tolist() == [9, 10, 11] and s.nodes[17][:3] == ("S", 13, 12)
    # a put split node keeps its plane and takes the new children
    put2 = np.zeros(1, node_dt)
    put2[0] = (2, 1, 0, 0, dense[15], dense[12], 0, 0, 0)
    s.apply_delta({"removed": np.array([dense[13]], np.uint32), "put_index": np.array([dense[17]], np.uint32), "put": put2,
                   "desc": np.zeros(0, np.uint32), "roots": np.array([dense[17]], np.uint32)}, dense)
    assert s.nodes[17] == ("S", 15, 12, hdr, vec) and s.roots == [17] and sorted(s.nodes) == [12, 15, 17]
