#!/usr/bin/env python3
"""Deleting items from a resident index against uploading the index again: what DESIGN.md §4 "Deletes on a resident index" reports.

One process, one forest.  Legs (seconds, median of `--reps` repetitions, each on an index of its own so that every repetition
deletes the same ids from the same forest):
  (a) ah_index_delete_items of `--deleted` ids; with AH_TIMING=1 in the environment the library prints the split into bitmap /
      levels / count / resolve / write / read-back on stderr for every repetition;
  (b) ah_index_create_from_view of that forest: the upload the routing step of an incremental build no longer needs.  A library
      without ah_index_delete_items (the parent commit) runs this leg only.
The bytes (a) has to move are computed from the forest: the stored ids are read by the count and the write pass and written
once, 4 bytes each; no normal is read.

    AH_TIMING=1 timeout 1100 python scripts/measure_index_delete.py --shape 10000000,768,100,cosine [--out profiles/index_delete.json]
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
    ap.add_argument("--deleted", type=int, default=10_000)
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
    ids = np.sort(np.random.default_rng(5).choice(n, a.deleted, replace=False)).astype(np.uint32)
    stored = int(view.descendants_len)
    out = {"shape": a.shape, "deleted": a.deleted, "nodes": int(view.n_nodes), "stored_ids": stored, "normal_bytes": int(view.normals_len),
           "delete_hbm_bytes": 3 * 4 * stored, "legs": {}}

    def leg(name, fn):
        t = []
        for rep in range(a.reps + 1):  # the first repetition warms the allocator and loads the kernels
            ix = Index(ds, None, view=view) if name == "delete" else None
            t0 = time.perf_counter()
            res = fn(ix)
            t.append(time.perf_counter() - t0)
            (ix or res).close()
        out["legs"][name] = {"median_s": statistics.median(t[1:]), "min_s": min(t[1:]), "max_s": max(t[1:]), "first_s": t[0]}
        print(name, out["legs"][name], flush=True)

    leg("create_from_view", lambda _ix: Index(ds, None, view=view))
    if hasattr(_lib.lib(), "ah_index_delete_items") and hasattr(Index, "delete_items"):
        leg("delete", lambda ix: ix.delete_items(ids, split_after))
        d = out["legs"]["delete"]["median_s"]
        out["delete_hbm_bytes_per_s"] = out["delete_hbm_bytes"] / d
        out["delete_below_create"] = d < out["legs"]["create_from_view"]["median_s"]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
