"""ah_index_encode_nodes without a GPU: the symbol and its declaration, and node_codec.values_of_export — the CPU restatement
the GPU tests (tests/test_gpu_index_encode.py) compare with — against node_codec.decode_value and against the Descendants
values roaring-rs wrote into tests/golden/large_v0_6.mdb."""
import os
import struct

import numpy as np

import node_codec_cases as cases
from conftest import ROOT

from arroy_amd import _lib, node_codec
from arroy_amd import distances as D
from arroy_amd.dataset import _NODE_DT


def test_the_library_exports_the_index_encode():
    lib = _lib.lib()
    assert "ah_index_encode_nodes" in _lib.SIGNATURES and lib.ah_index_encode_nodes is not None
    assert len(_lib.SIGNATURES["ah_index_encode_nodes"][1]) == 9
    with open(os.path.join(ROOT, "include", "arroy_hip.h")) as f:
        header = f.read()
    assert "ah_index_encode_nodes(" in header and "ah_index_encode_stats" in header
    assert lib.ah_abi_version() == 7  # an addition: the number stays
    # the struct as the header declares it: six counters and a double
    assert [f for f, _ in _lib.AhIndexEncodeStats._fields_] == ["n_values", "n_split", "n_descendants", "n_free", "value_bytes",
                                                                "pieces", "seconds"]
    import ctypes as C
    assert C.sizeof(_lib.AhIndexEncodeStats) == 56


def test_null_arguments_are_refused_without_a_device():
    import ctypes as C
    lib = _lib.lib()
    ends = (C.c_uint64 * 2)()
    assert lib.ah_index_encode_nodes(None, None, 0, None, 0, None, 0, ends, None) == 5 and b"index is NULL" in lib.ah_last_error()


def hand_made(dist, dims, rng):
    """An export dict by hand: slots 0 split (normal row 1), 1 Descendants, 2 free, 3 split `normal: None`, 4 an empty Descendants,
    5 a Descendants with a bitmap container, 6 split (row 0); the rows are padded as the device pads them."""
    hs, vs = dist.header_size(), dist.vector_size(dims)
    row_bytes = (vs + 127) // 128 * 128
    nodes = np.zeros(7, dtype=_NODE_DT)
    big = cases.edge_lists()["bitmap_array_one"]
    small = np.array([3, 9, 70000, 70001], np.uint32)
    desc = np.concatenate([small, big]).astype(np.uint32)
    nodes[0] = (2, 1, 0, 0, 1, 6, 1, 0, 0)
    nodes[1] = (1, 0, 0, 0, 0, 0, 0, small.size, 0)
    nodes[3] = (2, 0, 0, 0, 4, 5, 0, 0, 0)
    nodes[4] = (1, 0, 0, 0, 0, 0, small.size, 0, 0)
    nodes[5] = (1, 0, 0, 0, 0, 0, small.size, big.size, 0)
    nodes[6] = (2, 1, 0, 0, 3, 1, 0, 0, 0)
    rows = rng.integers(0, 256, size=(2, row_bytes), dtype=np.uint8)
    hdrs = rng.standard_normal((2, hs // 4)).astype(np.float32)
    export = {"nodes": nodes, "roots": np.array([0], np.uint32), "descendants": desc, "normal_rows": rows, "normal_headers": hdrs}
    return export, small, big


def test_values_of_export_round_trips_through_decode_value():
    rng = np.random.default_rng(11)
    for dist, dims in ((D.Euclidean, 32), (D.Manhattan, 30), (D.Cosine, 7), (D.DotProduct, 32), (D.BinaryQuantizedEuclidean, 70)):
        export, small, big = hand_made(dist, dims, rng)
        hs, vs = dist.header_size(), dist.vector_size(dims)
        id_of = np.array([10, 0xFFFFFFFE, 77, 5, 6, 0x01020304, 8], np.uint32)
        for table in (None, id_of):
            name = (lambda i: i) if table is None else (lambda i: int(table[i]))
            values = node_codec.values_of_export(export, dist, dims, table)
            assert len(values) == 7 and values[2] == b""
            dec = [node_codec.decode_value(dist, dims, v) if v else None for v in values]
            normal = [export["normal_headers"][r].tobytes() + export["normal_rows"][r].tobytes()[:vs] for r in (0, 1)]
            assert dec[0] == ("S", name(1), name(6), normal[1]) and len(values[0]) == 9 + hs + vs
            assert dec[6] == ("S", name(3), name(1), normal[0])
            assert dec[3] == ("S", name(4), name(5), None) and len(values[3]) == 9
            assert dec[1][0] == "D" and np.array_equal(dec[1][1], small)
            assert dec[4][0] == "D" and dec[4][1].size == 0 and len(values[4]) == 9
            assert dec[5][0] == "D" and np.array_equal(dec[5][1], big)
            assert values[5] == node_codec.encode_descendants(big) and len(values[5]) == 1 + 8 + 24 + 8192 + 8192 + 2
            assert values[0][1:9] == struct.pack(">II", name(1), name(6))


def test_values_of_export_reproduces_the_fixture_descendants():
    """The tag-1 tree values of large_v0_6.mdb (their layout has not changed up to v0.7; the fixture's split values have the
    v0.6 layout and are left out): an export whose slot i is the Descendants node of list i gives them back byte for byte."""
    values = cases.fixture_descendants()
    assert len(values) == 59
    lists = [node_codec.decode_value(D.Euclidean, 30, v)[1] for v in values]
    nodes = np.zeros(len(lists), dtype=_NODE_DT)
    at = 0
    for i, l in enumerate(lists):
        nodes[i] = (1, 0, 0, 0, 0, 0, at, len(l), 0)
        at += len(l)
    export = {"nodes": nodes, "roots": np.zeros(0, np.uint32), "descendants": np.concatenate(lists).astype(np.uint32),
              "normal_rows": np.zeros((0, 128), np.uint8), "normal_headers": np.zeros((0, 1), np.float32)}
    assert node_codec.values_of_export(export, D.Euclidean, 30, None) == values
