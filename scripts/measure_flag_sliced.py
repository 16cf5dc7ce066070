#!/usr/bin/env python3
"""Sliced duplicate flags against the sorted path: what DESIGN.md §4 "Sliced duplicate flags" reports.

One process, one index, one call of 1000 queries at count 100 and search_k 50 000 and 100 000: candidate strides of 65 536 and
131 072, past the one hash set of k_flag_duplicates_hash.  The index is the 10M x 768 Cosine one of 100 trees (ids past the LDS
bitmap) when the device holds it, otherwise the 1M x 1536 DotProduct one of 20 trees under AH_SEARCH_BITMAP=0.
AH_SEARCH_FLAG_SLICED alternates 0 / 1 call by call (0 launches what a library without the switch launches, so it is the
baseline), both settings warmed up first, `--calls` timed calls a setting.  Per search_k and setting: p50 / p99 / min / max of the
wall clock of the call (Python wrapper included; the call ends in a device synchronise) and the ah_search_stats of the timed
calls.  The spread inside a setting (max - min) is what a difference between the settings has to clear.

    timeout 900 python scripts/measure_flag_sliced.py [--shape 10000000,768,100] [--out profiles/flag_sliced.json]
    rocprofv3 --kernel-trace --stats -- python scripts/measure_flag_sliced.py --calls 5   (kernel time, a run of its own)
"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))

from arroy_amd import Dataset, _lib, shard  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

STATS = ("rerank_tiles", "rerank_sorted", "fallback_chunks", "fallback_select", "dedup_flag_hash", "tile_visits")


def build(shape):
    """(ds, forest, index, tunables of every call): the big index, or the benchmark's search index without the bitmap."""
    for (n, dims, trees), cls, tun in ((shape, D.Cosine, {}), ((1_000_000, 1536, 20), D.DotProduct, {"AH_SEARCH_BITMAP": 0})):
        ds = None
        try:
            ds = Dataset(cls, dims, n)
            ds.fill_synthetic(42, 1, n)
            if cls is D.DotProduct:
                ds.preprocess_dot()
            ds.finalize()
            forest = ds.build_forest(shard.tree_seeds(42, range(trees)))
            return ds, forest, ds.create_index(forest), tun, f"{n}x{dims} {cls.__name__}, {trees} trees" + ", AH_SEARCH_BITMAP=0" * bool(tun)
        except (MemoryError, RuntimeError) as e:  # the device does not hold it
            print(f"{n}x{dims}x{trees}: {e!r}", flush=True)
            if ds is not None:
                ds.close()
    raise SystemExit("no index could be built")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="10000000,768,100", help="n,dims,trees of the first index tried")
    ap.add_argument("--count", type=int, default=100)
    ap.add_argument("--search-k", default="50000,100000")
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=21, help="timed calls a setting")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls a setting and search_k")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ds, forest, index, tun, what = build(tuple(int(x) for x in a.shape.split(",")))
    rng = np.random.default_rng(5)
    rows = np.stack([ds.item_vector(int(i)) for i in rng.choice(len(ds), a.nq, replace=False)])
    queries = np.ascontiguousarray(rows + rng.standard_normal(rows.shape).astype(np.float32) * np.float32(0.05), dtype=np.float32)
    out = {"index": what, "count": a.count, "nq": a.nq, "calls": a.calls, "search_k": {}}
    print(f"index: {what}", flush=True)
    for sk in (int(x) for x in a.search_k.split(",")):
        t, stats, answers = {0: [], 1: []}, {0: dict.fromkeys(STATS, 0), 1: dict.fromkeys(STATS, 0)}, {}
        for rep in range(2 * (a.warmup + a.calls)):
            on = rep & 1
            index.stats(reset=True)
            with _lib.tuning(AH_SEARCH_FLAG_SLICED=on, **tun):
                t0 = time.perf_counter()
                got = index.search(a.count, queries=queries, search_k=sk, raw=True)
                dt = time.perf_counter() - t0
            if rep >= 2 * a.warmup:
                t[on].append(dt)
                st = index.stats()
                for k in STATS:
                    stats[on][k] += int(st[k])
            if rep < 2:  # the two settings answer alike: ids, distance bits, counts
                answers[on] = got
        assert all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
                   for x, y in zip(answers[0], answers[1])), f"search_k {sk}: the settings answer differently"
        out["search_k"][sk] = {}
        for on in (0, 1):
            print(f"search_k {sk:7d} switch {on}: ah_search_stats of its {a.calls} timed calls: " + ", ".join(f"{k} {v}" for k, v in stats[on].items()), flush=True)
            p50, p99 = np.percentile(t[on], [50, 99])
            out["search_k"][sk][f"switch {on}"] = {"p50_s": p50, "p99_s": p99, "min_s": min(t[on]), "max_s": max(t[on]), "calls": len(t[on]),
                                                    "qps": a.nq / p50, "stats_of_timed_calls": stats[on]}
            print(f"search_k {sk:7d} switch {on}: p50 {1e3 * p50:9.3f} ms  p99 {1e3 * p99:9.3f}  min {1e3 * min(t[on]):9.3f}  max {1e3 * max(t[on]):9.3f}  "
                  f"spread {1e3 * (max(t[on]) - min(t[on])):8.3f}  ({a.nq / p50:9.0f} queries/s)", flush=True)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    index.close()
    forest.close()
    ds.close()


if __name__ == "__main__":
    main()
