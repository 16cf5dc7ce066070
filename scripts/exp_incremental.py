#!/usr/bin/env python3
"""One incremental `Writer.build` with the resident index kept (`ArroyBuilder.device_insert`) against the same build ending with
an index made from a view of the whole store: what DESIGN.md §4 "Inserts and grafts on a resident index" reports.

One process, one `Database`.  A first build of `n` items, then `--updated` items are changed (half replaced, half new) and the
incremental build is timed.  Reported as one JSON line: the wall time of that build and the bytes its index calls copy from
the host to the device — the nodes (16 B each), ids and normal records of every view handed to ah_index_create_from_view or
ah_index_graft, and the ids of ah_index_insert_items / ah_index_delete_items / ah_route_items.  A library without
ah_index_insert_items (the parent commit) runs the same build on its only path.

    timeout 1100 python scripts/exp_incremental.py --shape 1000000,768,20,cosine --updated 4096 [--device-insert 0] [--out FILE]

With `--drop-trees K` the incremental build asks for K trees fewer than the first one built (`delete_extra_trees`), with
`--device-drop 1` on the resident index (`ArroyBuilder.device_drop`, Index.drop_trees), with 0 on the path without it: the index is
closed and one is made from the whole view afterwards.  What DESIGN.md §4 "Dropped trees on a resident index" reports.  `--timing 1`
sets AH_TIMING for the incremental build: the library's phase lines, the drop's among them, go to stderr.

    python scripts/exp_incremental.py --drop-trees 5 --device-drop 1 --timing 1
"""
import argparse
import json
import random
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))

from arroy_amd import _lib, dataset  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from arroy_amd import index as I  # noqa: E402

METRICS = {"cosine": D.Cosine, "dot": D.DotProduct, "euclidean": D.Euclidean}
copied = {"bytes": 0, "views": 0}


def view_bytes(v):
    return int(v.n_nodes) * 16 + int(v.n_trees) * 4 + int(v.descendants_len) * 4 + int(v.normals_len)


def count_copies():
    """wrap the Index calls that take host arrays: add what they hand to the device"""
    Index = dataset.Index
    init = Index.__init__

    def counted_init(self, ds, forest, view=None):
        if view is not None:
            copied["bytes"] += view_bytes(view)
            copied["views"] += 1
        init(self, ds, forest, view=view)
    Index.__init__ = counted_init
    if hasattr(Index, "drop_trees"):
        drop = Index.drop_trees

        def counted_drop(self, n_drop, sort_roots=False):
            t0 = time.perf_counter()
            out = drop(self, n_drop, sort_roots)
            copied["drop_s"] = time.perf_counter() - t0
            return out
        Index.drop_trees = counted_drop
    for name in ("route_items", "delete_items", "insert_items"):
        if not hasattr(Index, name):
            continue

        def make(fn):
            def counted(self, ids, *rest, **kw):
                copied["bytes"] += int(np.asarray(ids).size) * 4
                return fn(self, ids, *rest, **kw)
            return counted
        setattr(Index, name, make(getattr(Index, name)))
    if hasattr(Index, "graft"):
        graft = Index.graft

        def counted_graft(self, view, targets, new_index=None, want_map=False):
            copied["bytes"] += view_bytes(view) + int(view.n_nodes) * 8
            return graft(self, view, targets, new_index, want_map)
        Index.graft = counted_graft


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1000000,768,20,cosine", help="n,dims,trees,metric")
    ap.add_argument("--updated", type=int, default=4096)
    ap.add_argument("--device-insert", type=int, default=1)
    ap.add_argument("--drop-trees", type=int, default=0, help="the incremental build asks for this many trees fewer")
    ap.add_argument("--device-drop", type=int, default=0)
    ap.add_argument("--timing", type=int, default=0, help="AH_TIMING during the incremental build")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, dims, trees, metric = a.shape.split(",")
    n, dims, trees = int(n), int(dims), int(trees)
    count_copies()
    db = I.Database(METRICS[metric])
    w = I.Writer(db, 0, dims)
    rows = _lib.synth_rows_host(42, 1, n + a.updated, dims)
    for i in range(n):
        w.add_item(i, rows[i])
    t0 = time.perf_counter()
    w.builder(random.Random(1)).n_trees(trees).build()
    first_s = time.perf_counter() - t0
    g = np.random.default_rng(5)
    half = a.updated // 2
    for k, i in enumerate(g.choice(n, half, replace=False)):   # replaced
        w.add_item(int(i), rows[n + k])
    for k in range(a.updated - half):                          # new
        w.add_item(n + k, rows[n + half + k])
    b = w.builder(random.Random(2)).n_trees(max(0, trees - a.drop_trees))
    has = hasattr(b, "device_insert")
    if has:
        b.device_insert = bool(a.device_insert)
    has_drop = hasattr(b, "device_drop")
    if has_drop:
        b.device_drop = bool(a.device_drop)
    copied["bytes"], copied["views"] = 0, 0
    if a.timing:
        _lib.tuning_set("AH_TIMING", 1)
    t0 = time.perf_counter()
    b.build()
    build_s = time.perf_counter() - t0
    if a.timing:
        _lib.tuning_set("AH_TIMING", 0)
    st = w._st
    out = {"shape": a.shape, "updated": a.updated, "device_insert": bool(a.device_insert) if has else None, "first_build_s": first_s,
           "incremental_build_s": build_s, "host_to_device_bytes": copied["bytes"], "views_uploaded": copied["views"],
           "device_inserts": getattr(st, "device_inserts", None), "index_uploads": getattr(st, "index_uploads", None),
           "nodes": len(st.trees.nodes), "drop_trees": a.drop_trees, "device_drop": bool(a.device_drop) if has_drop else None,
           "device_drops": getattr(st, "device_drops", None), "drop_call_s": copied.get("drop_s"), "trees_after": len(st.trees.roots)}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    st.index.close()
    st.dataset.close()


if __name__ == "__main__":
    main()
