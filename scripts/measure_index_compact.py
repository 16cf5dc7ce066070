#!/usr/bin/env python3
"""Compacting a resident index against uploading it again: what DESIGN.md §4 "Compaction of a resident index" reports.

One process, one forest.  For every count in `--deleted` (seconds, median of `--reps` repetitions, each on an index of its own so
that every repetition compacts the same index):
  (a) ah_index_delete_items of that many ids (not timed here: scripts/measure_index_delete.py), then ah_index_compact; with
      AH_TIMING=1 in the environment the library prints the split into flags and scans / nodes / rows / swap on stderr for every
      repetition.  The time is the host's (the call synchronises before it swaps the pointers);
  (b) ah_index_create_from_view of the forest before the delete: the upload that was the only way to compact before (the forest
      after the delete is a little smaller, so this leg is a little long).
The bytes the row pass moves are computed from the footprint: the live rows and their headers, read once and written once.  The
copy rate of the box is what ah_bench_memcpy reports for a buffer of the size of the live rows (read + written bytes per second,
after one warm-up copy).

    AH_TIMING=1 timeout 1100 python scripts/measure_index_compact.py --shape 10000000,768,100,cosine [--out profiles/index_compact.json]
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))

from arroy_amd import Dataset, Index, _lib, shard  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

METRICS = {"cosine": D.Cosine, "dot": D.DotProduct, "euclidean": D.Euclidean}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="10000000,768,100,cosine", help="n,dims,trees,metric")
    ap.add_argument("--deleted", default="10000,1000000", help="ids deleted before the compaction, one leg per count")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, dims, trees, metric = a.shape.split(",")
    n, dims, trees = int(n), int(dims), int(trees)
    ds = Dataset(METRICS[metric], dims, n)
    ds.fill_synthetic(42, 1, n)
    if metric == "dot":
        ds.preprocess_dot()
    ds.finalize()
    forest = ds.build_forest(shard.tree_seeds(42, range(trees)))
    view = forest.view_struct()
    split_after = dims
    out = {"shape": a.shape, "nodes": int(view.n_nodes), "stored_ids": int(view.descendants_len), "legs": {}}

    def summary(t):  # the first repetition warms the allocator and loads the kernels
        return {"median_s": statistics.median(t[1:]), "min_s": min(t[1:]), "max_s": max(t[1:]), "first_s": t[0]}

    t = []
    for _rep in range(a.reps + 1):
        t0 = time.perf_counter()
        ix = Index(ds, None, view=view)
        t.append(time.perf_counter() - t0)
        ix.close()
    out["legs"]["create_from_view"] = summary(t)
    print("create_from_view", out["legs"]["create_from_view"], flush=True)
    for count in [int(c) for c in a.deleted.split(",")]:
        ids = np.sort(np.random.default_rng(5).choice(n, count, replace=False)).astype(np.uint32)
        t, fp, stats, geo = [], None, None, None
        for _rep in range(a.reps + 1):
            ix = Index(ds, None, view=view)
            ix.delete_items(ids, split_after)
            fp, geo = ix.footprint(), ix.export_info()
            t0 = time.perf_counter()
            stats = ix.compact()
            t.append(time.perf_counter() - t0)
            ix.close()
        leg = summary(t)
        moved = 2 * fp["live_normals"] * (geo["normal_row_bytes"] + 4 * geo["normal_header_floats"])
        leg.update({"footprint_before": fp, "stats": stats, "row_pass_bytes": moved, "bytes_per_s_whole_call": moved / leg["median_s"]})
        out["legs"][f"compact_after_{count}"] = leg
        print(f"compact_after_{count}", leg, flush=True)
    live_bytes = max(1 << 20, out["legs"][f"compact_after_{a.deleted.split(',')[0]}"]["row_pass_bytes"] // 2)
    _lib.bench_memcpy(0, live_bytes, 1)
    ms = _lib.bench_memcpy(0, live_bytes, 3)
    out["memcpy_bytes_per_s"] = 2 * live_bytes * 3 / (ms * 1e-3)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    forest.close()
    ds.close()


if __name__ == "__main__":
    main()
