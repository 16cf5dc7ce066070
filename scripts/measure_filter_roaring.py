#!/usr/bin/env python3
"""Filters from serialized RoaringBitmaps: what DESIGN.md §4 "Filters from serialized RoaringBitmaps" reports.

One process, one index (1M x 1536, 20 trees, as measure_filters.py).  64 candidate sets, each new to the library, at stored
shares 0.5, 0.05 and 0.001 (random ids: array and bitmap containers) and one clustered set of 64 (runs of ids: run containers
under cookie 12347).  Three ways to 64 resident filters, each timed as the filters alone and with the one 64-query
ah_search_batch_filters call that follows (query q under filter q); median of `--reps` repetitions after a warm-up:
  (a) the parent's way: the host expands every serialized bitmap into dense words (timed apart: "host expansion"), then
      64 x ah_filter_create_bitmap;
  (b) 64 x ah_filter_create_roaring;
  (c) one ah_filter_create_roaring_batch.
A library without the roaring symbols (the parent commit) runs (a) only.

    timeout 900 python scripts/measure_filter_roaring.py [--shape 1000000,1536,20,dot] [--out profiles/filter_roaring.json]
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))

from arroy_amd import Dataset, _lib, roaring, shard  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

METRICS = {"cosine": D.Cosine, "dot": D.DotProduct, "euclidean": D.Euclidean}


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def words_of(blob, n):
    """The host's half of way (a): the serialized bitmap as dense uint64 words over [0, n)."""
    ids = roaring.deserialize(blob)
    bits = np.zeros((n + 63) // 64 * 64, np.bool_)
    bits[ids[ids < n]] = True
    return np.packbits(bits, bitorder="little").view(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1000000,1536,20,dot", help="n,dims,trees,metric")
    ap.add_argument("--count", type=int, default=100)
    ap.add_argument("--search-k", type=int, default=10_000)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
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
    index = ds.create_index(forest)
    have = hasattr(_lib.lib(), "ah_filter_create_roaring_batch") and hasattr(index, "make_filters_roaring")
    rng = np.random.default_rng(5)
    nf = a.filters
    queries = _lib.synth_rows_host(42, 1, nf, dims, first_item=0) + rng.standard_normal((nf, dims)).astype(np.float32) * np.float32(0.05)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    slots = np.arange(nf, dtype=np.uint32)
    kw = dict(search_k=a.search_k, raw=True)
    out = {"shape": a.shape, "count": a.count, "search_k": a.search_k, "filters": nf, "reps": a.reps, "roaring_symbols": bool(have), "legs": {}}

    def note(name, sec, extra=None):
        med, lo, hi = sec
        out["legs"][name] = {"median_ms": 1e3 * med, "min_ms": 1e3 * lo, "max_ms": 1e3 * hi, **(extra or {})}
        print(f"{name:64s} {1e3 * med:9.3f} ms  (min {1e3 * lo:.3f} max {1e3 * hi:.3f})", flush=True)

    def search_and_close(filters):
        index.search(a.count, queries=queries, filters=filters, filter_of_query=slots, **kw)
        for f in filters:
            f.close()

    def close(filters):
        for f in filters:
            f.close()

    sets = []
    for share in (0.5, 0.05, 0.001):
        sets.append((f"share {share}", False, [np.sort(rng.choice(n, int(n * share), replace=False)).astype(np.uint32) for _ in range(nf)]))
    clustered = []
    for _ in range(nf):  # 200 runs of 500 .. 1500 ids: share about 0.2, run containers
        starts = np.sort(rng.choice(n - 2000, 200, replace=False))
        clustered.append(np.unique(np.concatenate([np.arange(s, s + int(rng.integers(500, 1500))) for s in starts])).astype(np.uint32))
    sets.append(("clustered runs", True, clustered))
    for tag, runs, lists in sets:
        blobs = [roaring.serialize(x, runs=runs) for x in lists]
        size = {"blob_bytes_mean": float(np.mean([len(b) for b in blobs])), "ids_mean": float(np.mean([x.size for x in lists]))}
        print(f"-- {tag}: {size['ids_mean']:.0f} ids and {size['blob_bytes_mean']:.0f} serialized bytes a set", flush=True)
        note(f"{tag}: (a) host expansion of {nf} blobs to words", timed(lambda: [words_of(b, n) for b in blobs], max(3, a.reps // 2), warmup=1), size)
        words = [words_of(b, n) for b in blobs]
        note(f"{tag}: (a) {nf} x ah_filter_create_bitmap", timed(lambda: close([index.make_filter_bitmap(w, n) for w in words]), a.reps))
        note(f"{tag}: (a) {nf} x ah_filter_create_bitmap + search", timed(lambda: search_and_close([index.make_filter_bitmap(w, n) for w in words]), a.reps))
        if not have:
            continue
        note(f"{tag}: (b) {nf} x ah_filter_create_roaring", timed(lambda: close([index.make_filter_roaring(b) for b in blobs]), a.reps))
        note(f"{tag}: (b) {nf} x ah_filter_create_roaring + search", timed(lambda: search_and_close([index.make_filter_roaring(b) for b in blobs]), a.reps))
        filters, st = index.make_filters_roaring(blobs)
        close(filters)
        note(f"{tag}: (c) one ah_filter_create_roaring_batch", timed(lambda: close(index.make_filters_roaring(blobs)[0]), a.reps), {"stats": st})
        note(f"{tag}: (c) one ah_filter_create_roaring_batch + search", timed(lambda: search_and_close(index.make_filters_roaring(blobs)[0]), a.reps))
    note(f"the {nf}-query search alone, unfiltered", timed(lambda: index.search(a.count, queries=queries, **kw), a.reps))
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    index.close()
    forest.close()
    ds.close()


if __name__ == "__main__":
    main()
