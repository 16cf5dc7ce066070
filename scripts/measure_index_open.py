#!/usr/bin/env python3
"""Opening a resident index from the bytes LMDB stores: what DESIGN.md §4 "Opening a resident index from encoded nodes" reports.

A synthetic Cosine dataset (`--rows` x `--dims`), `--trees` trees; the `NodeCodec` values of its forest are taken from
ah_build_forest_stream_encoded and kept in host memory as a cursor would yield them, ascending by node id.  Seconds, median of
`--reps` repetitions after one warm-up:
  (a) today's path: every value decoded on one host thread by the serial functions of csrc/node_decode.h into the arrays of an
      ah_forest_view (scripts/measure_index_open_host.cpp, compiled here with -O2), then ah_index_create_from_view;
  (b) ah_index_create_from_encoded;
  (c) of (b), the host's copy of the values into pinned memory (ah_index_decode_stats.seconds_host_copy).
The two indexes are compared array for array once.

    timeout -k 10 600 python scripts/measure_index_open.py [--rows 1000000 --dims 768 --trees 20] [--out profiles/index_open.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from arroy_amd import Dataset, Index, _lib, shard  # noqa: E402
from arroy_amd import distances as D  # noqa: E402


class HostView(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("roots", C.c_void_p), ("descendants", C.c_void_p), ("normals", C.c_void_p),
                ("n_nodes", C.c_uint64), ("descendants_len", C.c_uint64), ("normals_len", C.c_uint64), ("normal_stride", C.c_uint64),
                ("n_trees", C.c_uint32), ("bad_reason", C.c_uint32), ("bad_position", C.c_uint64)]


def build_host_decoder(tmp):
    so = os.path.join(tmp, "measure_index_open_host.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-shared", "-fPIC", "-fvisibility=hidden",
                           os.path.join(ROOT, "scripts", "measure_index_open_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.host_view_decode.restype = C.c_int
    lib.host_view_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64,
                                     C.POINTER(HostView)]
    lib.host_view_free.restype = None
    lib.host_view_free.argtypes = [C.POINTER(HostView)]
    return lib


class Values:
    """The sink of the encoded stream: every batch's payload copied as it arrives, node ids and value extents kept as arrays."""

    def __init__(self):
        self.keep, self.ids, self.ptrs, self.lens = [], [], [], []
        self.node_dt = np.dtype(_lib.AhStreamNode)

    def take(self, b):
        n = int(b.n_nodes)
        if n == 0:
            return 0
        nodes = np.frombuffer(C.string_at(b.nodes, n * self.node_dt.itemsize), dtype=self.node_dt)
        pay = np.ctypeslib.as_array(b.payload, shape=(int(b.payload_len),)).copy()
        off = nodes["payload_offset"].astype(np.uint64)
        self.keep.append(pay)
        self.ids.append(nodes["id"].astype(np.uint32))
        self.ptrs.append(off + np.uint64(pay.ctypes.data))
        self.lens.append(np.diff(np.append(off, np.uint64(b.payload_len))))
        return 0

    def sorted(self):
        ids, ptrs, lens = np.concatenate(self.ids), np.concatenate(self.ptrs), np.concatenate(self.lens)
        order = np.argsort(ids, kind="stable")
        return (np.ascontiguousarray(ids[order]), np.ascontiguousarray(ptrs[order].astype(np.uint64)),
                np.ascontiguousarray(lens[order].astype(np.uint64)))


def timed(fn, reps, cleanup):
    t, res = [], None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        res = fn()
        t.append(time.perf_counter() - t0)
        if r < reps:
            cleanup(res)
    return statistics.median(t[1:]), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    dist = D.Cosine
    t0 = time.perf_counter()
    ds = Dataset(dist, a.dims, a.rows)
    ds.fill_synthetic(42, 1, a.rows)
    ds.finalize()
    sink = Values()
    roots, _stats, _none = ds.build_forest_stream(shard.tree_seeds(42, range(a.trees)), sink=sink.take, encoded=True, node_id_base=0x01020304)
    ids, ptrs, lens = sink.sorted()
    n = ids.size
    print(f"staged, built and collected {n} values in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    hs, vs = dist.header_size(), dist.vector_size(a.dims)

    with tempfile.TemporaryDirectory() as tmp:
        host = build_host_decoder(tmp)

        def leg_a():
            hv = HostView()
            t = time.perf_counter()
            assert host.host_view_decode(ids.ctypes.data, ptrs.ctypes.data, lens.ctypes.data, n, roots.ctypes.data, roots.size, hs, vs,
                                         C.byref(hv)) == 0, (hv.bad_position, hv.bad_reason)
            decode_s = time.perf_counter() - t
            v = _lib.AhForestView()
            v.n_trees, v.n_nodes = hv.n_trees, hv.n_nodes
            v.roots = C.cast(hv.roots, C.POINTER(C.c_uint32))
            v.nodes = C.cast(hv.nodes, C.POINTER(_lib.AhNode))
            v.normals = C.cast(hv.normals, C.POINTER(C.c_uint8))
            v.normals_len, v.normal_stride, v.normal_vector_offset, v.normal_header_offset = hv.normals_len, hv.normal_stride, hs, 0
            v.descendants = C.cast(hv.descendants, C.POINTER(C.c_uint32))
            v.descendants_len = hv.descendants_len
            ix = Index(ds, None, view=v)
            host.host_view_free(C.byref(hv))
            return ix, decode_s

        def leg_b():
            h, st = C.c_void_p(), _lib.AhIndexDecodeStats()
            _lib.check(L.ah_index_create_from_encoded(ds._h, ids.ctypes.data, ptrs.ctypes.data_as(C.POINTER(C.c_void_p)),
                                                      lens.ctypes.data_as(C.POINTER(C.c_size_t)), n, roots.ctypes.data, roots.size,
                                                      C.byref(h), C.byref(st)))
            ix = Index.__new__(Index)
            ix.dataset, ix._h, ix._filters = ds, h, set()
            return ix, st

        decode_times, copy_times = [], []

        def run_a():
            ix, s = leg_a()
            decode_times.append(s)
            return ix

        def run_b():
            ix, st = leg_b()
            copy_times.append(st.seconds_host_copy)
            run_b.stats = st
            return ix

        sa, ia = timed(run_a, a.reps, lambda ix: ix.close())
        sb, ib = timed(run_b, a.reps, lambda ix: ix.close())
        st = run_b.stats
        ea, eb = ia.export(), ib.export()
        same = ia.export_info() == ib.export_info() and all(ea[k].tobytes() == eb[k].tobytes() for k in ea)
        ia.close()
        ib.close()
    lines = [
        f"# python scripts/measure_index_open.py --rows {a.rows} --dims {a.dims} --trees {a.trees} --reps {a.reps}",
        f"# {_lib.device_name(0)}: {a.rows} rows x {a.dims} dims, Cosine, {a.trees} trees: {n} values, {int(lens.sum())} bytes "
        f"({int(st.split_values)} split values, {int(st.normals)} with a plane, {int(st.descendants_values)} Descendants values of {int(st.ids)} ids "
        f"in {int(st.containers_array)} array / {int(st.containers_bitmap)} bitmap / {int(st.containers_run)} run containers; "
        f"{int(st.chunks)} chunks, {int(st.bytes_staged)} bytes staged); seconds, median of {a.reps} after one warm-up",
        f"(a) serial host decode into a view + ah_index_create_from_view: {sa:.4f} s  (the decode alone {statistics.median(decode_times[1:]):.4f} s)",
        f"(b) ah_index_create_from_encoded: {sb:.4f} s",
        f"(c) of (b), the host copy into pinned memory: {statistics.median(copy_times[1:]):.4f} s",
        f"(a) / (b) = {sa / sb:.2f}; the two indexes are {'equal' if same else 'NOT EQUAL'} array for array",
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
