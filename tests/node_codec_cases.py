"""Id lists the node codec tests share (tests/test_node_codec_cpu.py, tests/test_gpu_node_codec.py): the Descendants
values roaring-rs wrote into tests/golden/large_v0_6.mdb, and lists at every edge of the container rules."""
import importlib.util
import os
import struct

import numpy as np

from conftest import ROOT

MDB = os.path.join(ROOT, "tests", "golden", "large_v0_6.mdb")


def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fixture_descendants():
    """The tag-1 values among the tree nodes (key mode 2) of large_v0_6.mdb, in key order: real RoaringBitmap::serialize_into
    output (Descendants values have not changed since v0.4, src/node.rs:357-361)."""
    out = []
    for key, val in _make_golden().parse_mdb(MDB):
        _index, mode, _node = struct.unpack(">HBI", key[:7])
        if mode == 2 and val and val[0] == 1:
            out.append(bytes(val))
    return out


def edge_lists():
    """name -> ascending u32 ids; every id below 2^20."""
    rng = np.random.default_rng(20240611)
    many = np.sort(rng.choice(1 << 20, size=900, replace=False)).astype(np.uint32)  # 16 containers of ~56 ids
    return {
        "empty": np.zeros(0, np.uint32),
        "one": np.array([7], np.uint32),
        "array_4096": np.arange(0, 2 * 4096, 2, dtype=np.uint32) + np.uint32(3 << 16),           # the largest array container
        "bitmap_4097": np.arange(0, 3 * 4097, 3, dtype=np.uint32) + np.uint32(5 << 16),          # the smallest bitmap container
        "neighbours_65535_65536": np.array([65535, 65536], np.uint32),
        "bitmap_array_one": np.concatenate([np.arange(100, 100 + 4097), (1 << 16) + np.arange(0, 4096 * 5, 5),
                                            [(9 << 16) + 65535]]).astype(np.uint32),
        "full_container": np.arange(2 << 16, 3 << 16, dtype=np.uint32),
        "spread_900": many,
        "wave_edges": np.concatenate([np.arange(63), [65536 + 1], 131072 + np.arange(65), [196608]]).astype(np.uint32),
    }


def containers_300():
    """300 containers, 1 to 3 ids each: ids up to 300 * 65536 (the host encoders only; the device tests stay below 2^20)."""
    rng = np.random.default_rng(5)
    parts = [np.sort(rng.choice(65536, size=1 + k % 3, replace=False)) + (k << 16) for k in range(300)]
    return np.concatenate(parts).astype(np.uint32)
