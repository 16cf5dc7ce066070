"""What the tests of the v0.4 - v0.6 node layouts share (tests/test_node_legacy_cpu.py, tests/test_gpu_index_legacy.py): the tree
values and items of the two v0.6 fixtures, the reference's expected dumps, and the rewriting of v0.7 values into the old layout."""
import json
import os
import struct

import numpy as np

from conftest import ROOT
from node_codec_cases import _make_golden

from arroy_amd import node_codec

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = {"smol": ("smol_v0_6.mdb", 2), "large": ("large_v0_6.mdb", 30)}  # name -> (file, dimensions); both Euclidean


def fixture(name):
    """(dims, item ids, item vectors f32 [n, dims], tree node ids, tree values, roots) of a fixture, in key order."""
    path, dims = FIXTURES[name]
    item_ids, vectors, node_ids, values = [], [], [], []
    for key, val in _make_golden().parse_mdb(os.path.join(GOLDEN, path)):
        _index, mode, node = struct.unpack(">HBI", key[:7])
        if mode == 3:
            assert val[0] == 0 and len(val) == 5 + 4 * dims
            item_ids.append(node)
            vectors.append(np.frombuffer(val, dtype="<f4", offset=5, count=dims))
        elif mode == 2:
            node_ids.append(node)
            values.append(bytes(val))
    return dims, item_ids, np.stack(vectors).astype(np.float32), node_ids, values, expected()[name]["roots"]


def expected():
    with open(os.path.join(GOLDEN, "upgrade_expected.json")) as f:
        return json.load(f)


def records(distance, dims, node_ids, values):
    """v0.7 values in the shape of upgrade_expected.json: {str(node id): record}."""
    out = {}
    for nid, v in zip(node_ids, values):
        d = node_codec.decode_value(distance, dims, v)
        if d[0] == "S":
            out[str(int(nid))] = {"kind": "split", "left": d[1], "right": d[2], "normal": d[3] is not None}
        else:
            out[str(int(nid))] = {"kind": "descendants", "descendants": d[1].tolist()}
    return out


def fold_to_legacy(layout, node_ids, values, distance, dims):
    """v0.7 values rewritten into a legacy layout: every Descendants node of exactly one id whose parent is a split node is
    folded into an Item child and its value dropped; every `normal: None` becomes a zero vector, every tenth of them written as
    -0.0 for the f32 codecs; the header of a normal is dropped.  -> (node ids, legacy values, the counts folded)."""
    hs, vs = distance.header_size(), distance.vector_size(dims)
    dec = {int(n): node_codec.decode_value(distance, dims, v) for n, v in zip(node_ids, values)}
    folded = set()
    for nid, d in dec.items():
        if d[0] == "S":
            folded.update(c for c in d[1:3] if dec[c][0] == "D" and dec[c][1].size == 1)
    counts = dict(split_values=0, zero_normals=0, headers_made=0, item_children=0, left_items=0, right_items=0, both_items=0, minus_zero=0)
    out_ids, out_values = [], []
    for nid, value in zip(node_ids, values):
        nid, d = int(nid), dec[int(nid)]
        if nid in folded:
            continue
        out_ids.append(nid)
        if d[0] == "D":
            out_values.append(bytes(value))
            continue
        children = [("item", int(dec[c][1][0])) if c in folded else ("tree", c) for c in d[1:3]]
        n_items = sum(m == "item" for m, _ in children)
        counts["split_values"] += 1
        counts["item_children"] += n_items
        counts["left_items"] += children[0][0] == "item"
        counts["right_items"] += children[1][0] == "item"
        counts["both_items"] += n_items == 2
        if d[3] is None:
            vector = b"\0" * vs
            if not distance.binary_quantized and counts["zero_normals"] % 10 == 9:
                vector = struct.pack("<f", -0.0) * (vs // 4)
                counts["minus_zero"] += 1
            counts["zero_normals"] += 1
        else:
            vector = d[3][hs:]
            counts["headers_made"] += 1
        out_values.append(node_codec.encode_split_legacy(layout, children[0], children[1], vector))
    counts["new_nodes"] = counts["item_children"]
    return out_ids, out_values, counts
