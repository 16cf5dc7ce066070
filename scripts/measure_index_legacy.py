#!/usr/bin/env python3
"""Opening a resident index from the v0.4 - v0.6 node bytes: what DESIGN.md §4 "Opening a resident index from the v0.4 - v0.6
node bytes" reports.

A synthetic Cosine dataset (`--rows` x `--dims`), `--trees` trees; the v0.7 `NodeCodec` values of its forest are taken from
ah_build_forest_stream_encoded and rewritten into the v0.6 layout as tests/test_gpu_index_legacy.py does (every one-id
Descendants node below a split node folded into an Item child, every `normal: None` a zero vector, no headers).
Milliseconds, median of `--reps` opens after one warm-up, every call on pointer arrays prepared beforehand:
  legacy  ah_index_create_from_legacy(AH_NODE_LAYOUT_V0_5) on the rewritten values;
  (a)     ah_index_create_from_encoded on the v0.7 values of the same forest;
  (b)     the host route: node_codec.upgrade_values on the CPU (once; its seconds are reported), then (a) on its values.
The legacy index is compared array for array with (b)'s once.

    timeout -k 10 900 python scripts/measure_index_legacy.py [--rows 1000000 --dims 768 --trees 20] [--out profiles/index_legacy.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import node_legacy_cases as legacy_cases  # noqa: E402

from arroy_amd import Dataset, Index, _lib, node_codec, shard  # noqa: E402
from arroy_amd import distances as D  # noqa: E402


def collect(ds, trees):
    """(node ids, values as bytes, roots) of an encoded build, ascending by node id."""
    got = {}
    node_dt = np.dtype(_lib.AhStreamNode)

    def take(b):
        n = int(b.n_nodes)
        if n:
            nodes = np.frombuffer(C.string_at(b.nodes, n * node_dt.itemsize), dtype=node_dt)
            pay = C.string_at(b.payload, int(b.payload_len))
            off = nodes["payload_offset"].astype(np.int64).tolist() + [int(b.payload_len)]
            for i, nid in enumerate(nodes["id"].tolist()):
                got[nid] = pay[off[i]: off[i + 1]]
        return 0
    roots, _stats, _none = ds.build_forest_stream(shard.tree_seeds(42, range(trees)), sink=take, encoded=True, node_id_base=0x01020304)
    ids = sorted(got)
    return ids, [got[i] for i in ids], [int(r) for r in roots]


class Call:
    """The arguments of one open, prepared once: the timed region is the library call alone."""

    def __init__(self, ds, node_ids, values, roots, layout):
        self.ds, self.layout, self.n = ds, layout, len(node_ids)
        self.keep = [np.frombuffer(v, dtype=np.uint8) for v in values]
        self.ids = np.array(node_ids, dtype=np.uint32)
        self.ptrs = np.array([a.ctypes.data for a in self.keep], dtype=np.uint64)
        self.lens = np.array([a.size for a in self.keep], dtype=np.uint64)
        self.roots = np.array(roots, dtype=np.uint32)
        self.legacy = _lib.AhIndexLegacyStats()

    def __call__(self):
        h = C.c_void_p()
        args = (self.ids.ctypes.data, self.ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), self.lens.ctypes.data_as(C.POINTER(C.c_size_t)), self.n,
                self.roots.ctypes.data, self.roots.size, C.byref(h), None)
        if self.layout == _lib.NODE_LAYOUT_V0_7:
            _lib.check(_lib.lib().ah_index_create_from_encoded(self.ds._h, *args))
        else:
            _lib.check(_lib.lib().ah_index_create_from_legacy(self.ds._h, self.layout, *args, C.byref(self.legacy)))
        ix = Index.__new__(Index)
        ix.dataset, ix._h, ix._filters = self.ds, h, set()
        return ix


def timed_ms(call, reps):
    t, ix = [], None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        ix = call()
        t.append(1e3 * (time.perf_counter() - t0))
        if r < reps:
            ix.close()
    return statistics.median(t[1:]), ix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dist = D.Cosine
    t0 = time.perf_counter()
    ds = Dataset(dist, a.dims, a.rows)
    ds.fill_synthetic(42, 1, a.rows)
    ds.finalize()
    node_ids, values, roots = collect(ds, a.trees)
    print(f"staged, built and collected {len(values)} values in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    old_ids, old_values, counts = legacy_cases.fold_to_legacy("v0.6", node_ids, values, dist, a.dims)
    print(f"rewritten into the v0.6 layout in {time.perf_counter() - t0:.1f} s: {counts}", file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    up_ids, up_values, _put = node_codec.upgrade_values("v0.6", old_ids, old_values, dist, a.dims)
    host_upgrade_s = time.perf_counter() - t0
    print(f"node_codec.upgrade_values on the CPU: {host_upgrade_s:.1f} s", file=sys.stderr, flush=True)

    legacy_call = Call(ds, old_ids, old_values, roots, _lib.NODE_LAYOUT_V0_5)
    ms_legacy, ix_legacy = timed_ms(legacy_call, a.reps)
    ms_a, ix_a = timed_ms(Call(ds, node_ids, values, roots, _lib.NODE_LAYOUT_V0_7), a.reps)
    ix_a.close()
    ms_b, ix_b = timed_ms(Call(ds, up_ids, up_values, roots, _lib.NODE_LAYOUT_V0_7), a.reps)
    el, eb = ix_legacy.export(), ix_b.export()
    same = ix_legacy.export_info() == ix_b.export_info() and all(el[k].tobytes() == eb[k].tobytes() for k in el)
    ix_legacy.close()
    ix_b.close()
    lg = legacy_call.legacy
    lines = [
        f"# python scripts/measure_index_legacy.py --rows {a.rows} --dims {a.dims} --trees {a.trees} --reps {a.reps}",
        f"# {_lib.device_name(0)}: {a.rows} rows x {a.dims} dims, Cosine, {a.trees} trees: {len(values)} v0.7 values of {sum(map(len, values))} bytes, "
        f"{len(old_values)} v0.6 values of {sum(map(len, old_values))} bytes ({int(lg.split_values)} split values, {int(lg.zero_normals)} zero normals, "
        f"{int(lg.headers_made)} headers made, {int(lg.item_children)} Item children); milliseconds, median of {a.reps} opens after one warm-up",
        f"legacy  ah_index_create_from_legacy on the v0.6 values: {ms_legacy:.2f} ms",
        f"(a)     ah_index_create_from_encoded on the v0.7 values of the same forest: {ms_a:.2f} ms",
        f"(b)     node_codec.upgrade_values on the CPU ({1e3 * host_upgrade_s:.0f} ms) + ah_index_create_from_encoded on its values ({ms_b:.2f} ms): "
        f"{1e3 * host_upgrade_s + ms_b:.0f} ms",
        f"legacy / (a) = {ms_legacy / ms_a:.2f}; the legacy index and (b)'s are {'equal' if same else 'NOT EQUAL'} array for array",
    ]
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ds.close()
    assert same


if __name__ == "__main__":
    main()
