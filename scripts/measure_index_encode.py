#!/usr/bin/env python3
"""Values of an incremental build from the resident index: what DESIGN.md §4 "Encoded values from a resident index" reports.

A synthetic Cosine dataset (`--rows` x `--dims`), `--trees` trees, resident as an Index.  `--share` of the items are deleted
(ah_index_delete_items) and inserted again (ah_index_insert_items).  For each of the two deltas, seconds, median of `--reps`
repetitions after one warm-up:
  (a) ah_index_encode_nodes on the delta's put nodes (the sizes call and the values call together);
  (b) ah_encode_descendants on the Descendants lists of the same delta, uploaded from the host (both calls);
  (c) the plain-C host encoder of examples/stream_encoded.c on the same lists, one thread.
(b) and (c) encode the lists only; (a) also the put split nodes, whose normals (b) and (c) would have to read back from the
store.  The Descendants values of (a) are compared with (b)'s once.  Then (d): ah_index_encode_nodes of every node slot.

    timeout -k 10 600 python scripts/measure_index_encode.py [--rows 1000000 --dims 768 --trees 20] [--out profiles/index_encode.txt]
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


def build_host_encoder(tmp):
    so = os.path.join(tmp, "measure_index_encode_host.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-O2", "-shared", "-fPIC", "-D_POSIX_C_SOURCE=200809L",
                           "-Dmain=stream_encoded_main", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "scripts", "measure_index_encode_host.c"), "-o", so,
                           "-L", os.path.join(ROOT, "arroy_amd"), "-larroy_hip", "-ldl",  # (the example's own main calls the library)
                           f"-Wl,-rpath,{os.path.join(ROOT, 'arroy_amd')}", "-Wl,-rpath,/opt/rocm/lib"])
    lib = C.CDLL(so)
    lib.host_encode_lists.restype = C.c_int
    lib.host_encode_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    return lib


def median_of(fn, reps):
    t, res = [], None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        res = fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t[1:]), res


def encode_nodes(ix, idx):
    """The two calls a host makes: sizes, then values.  -> (offsets, bytes, stats of the values call)"""
    L = _lib.lib()
    n = ix.export_info()["n_nodes"] if idx is None else idx.size
    ends = np.zeros(n + 1, dtype=np.uint64)
    st = _lib.AhIndexEncodeStats()
    p = None if idx is None else idx.ctypes.data
    _lib.check(L.ah_index_encode_nodes(ix._h, p, n, None, 0, None, 0, ends.ctypes.data, None))
    out = np.empty(max(1, int(ends[n])), dtype=np.uint8)
    _lib.check(L.ah_index_encode_nodes(ix._h, p, n, None, 0, out.ctypes.data, out.size, ends.ctypes.data, C.byref(st)))
    return ends, out, st


def encode_lists(ds, ids, offsets):
    L = _lib.lib()
    n = offsets.size - 1
    ends = np.zeros(n + 1, dtype=np.uint64)
    _lib.check(L.ah_encode_descendants(ds._h, ids.ctypes.data, offsets.ctypes.data, n, None, 0, ends.ctypes.data))
    out = np.empty(max(1, int(ends[n])), dtype=np.uint8)
    _lib.check(L.ah_encode_descendants(ds._h, ids.ctypes.data, offsets.ctypes.data, n, out.ctypes.data, out.size, ends.ctypes.data))
    return ends, out


def delta_legs(name, ix, ds, delta, host, reps):
    put_index = np.ascontiguousarray(delta["put_index"], dtype=np.uint32)
    put = delta["put"]
    leaves = np.flatnonzero(put["kind"] == 1)
    counts = put["count"][leaves].astype(np.uint64)
    offsets = np.zeros(leaves.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts)
    desc = delta["desc"]
    ids = np.concatenate([desc[int(o):int(o) + int(c)] for o, c in zip(put["offset"][leaves], counts)]).astype(np.uint32) \
        if leaves.size else np.zeros(1, np.uint32)
    sa, (ends_a, out_a, st) = median_of(lambda: encode_nodes(ix, put_index), reps)
    sb, (ends_b, out_b) = median_of(lambda: encode_lists(ds, ids, offsets), reps)
    host_s, host_bytes = [], C.c_uint64()
    for _ in range(reps + 1):
        s = C.c_double()
        assert host.host_encode_lists(ids.ctypes.data, offsets.ctypes.data, leaves.size, C.byref(host_bytes), C.byref(s)) == 0
        host_s.append(s.value)
    sc = statistics.median(host_s[1:])
    same = all(out_a[int(ends_a[i]):int(ends_a[i + 1])].tobytes() == out_b[int(ends_b[k]):int(ends_b[k + 1])].tobytes()
               for k, i in enumerate(leaves)) and int(host_bytes.value) == int(ends_b[-1])
    lines = [
        f"{name}: {put_index.size} put nodes ({int(st.n_descendants)} Descendants of {int(offsets[-1])} ids, {int(st.n_split)} split), "
        f"{int(st.value_bytes)} bytes of values in {int(st.pieces)} pieces",
        f"  (a) ah_index_encode_nodes on the put nodes: {sa:.4f} s  (the values call alone {st.seconds:.4f} s)",
        f"  (b) ah_encode_descendants on the {leaves.size} lists from the host: {sb:.4f} s",
        f"  (c) host C encoder (examples/stream_encoded.c) on the {leaves.size} lists: {sc:.4f} s",
        f"  the Descendants values of (a) and (b) are {'equal' if same else 'NOT EQUAL'}",
    ]
    return lines, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--share", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t0 = time.perf_counter()
    ds = Dataset(D.Cosine, a.dims, a.rows)
    ds.fill_synthetic(42, 1, a.rows)
    ds.finalize()
    seeds = shard.tree_seeds(42, range(a.trees))
    forest = ds.build_forest(seeds)
    ix = Index(ds, forest)
    forest.close()
    print(f"staged, built and mirrored in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    changed = np.sort(np.random.default_rng(1).choice(a.rows, size=max(1, int(a.rows * a.share)), replace=False)).astype(np.uint32)
    lines = [
        f"# python scripts/measure_index_encode.py --rows {a.rows} --dims {a.dims} --trees {a.trees} --share {a.share} --reps {a.reps}",
        f"# {_lib.device_name(0)}: {a.rows} rows x {a.dims} dims, Cosine, {a.trees} trees, {ix.export_info()['n_nodes']} nodes; "
        f"{changed.size} items deleted, then inserted again; seconds, median of {a.reps} after one warm-up, AH_READBACK_MB="
        f"{_lib.tuning_get('AH_READBACK_MB')[0]}",
    ]
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        host = build_host_encoder(tmp)
        for name, step in (("delete", lambda: ix.delete_items(changed, a.dims)), ("insert", lambda: ix.insert_items(changed, seeds))):
            t1 = time.perf_counter()
            delta = step()
            lines.append(f"ah_index_{name}_items with its delta: {time.perf_counter() - t1:.4f} s (once)")
            more, same = delta_legs(name, ix, ds, delta, host, a.reps)
            lines += more
            ok = ok and same
    sd, (ends, _out, st) = median_of(lambda: encode_nodes(ix, None), a.reps)
    lines.append(f"(d) ah_index_encode_nodes of every node slot: {sd:.4f} s  ({int(st.n_values)} slots, {int(st.n_free)} free, "
                 f"{int(st.n_split)} split, {int(st.n_descendants)} Descendants; {int(st.value_bytes)} bytes in {int(st.pieces)} pieces; "
                 f"the values call alone {st.seconds:.4f} s)")
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ix.close()
    ds.close()
    assert ok


if __name__ == "__main__":
    main()
