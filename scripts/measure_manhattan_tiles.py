#!/usr/bin/env python3
"""Manhattan's exact leaf tiles against the sorted path: what DESIGN.md §4 "Manhattan leaf tiles" reports.

One process, one index (1M x 768 Manhattan, 20 trees), one call of 1000 queries at search_k 10 000, count 100.
AH_SEARCH_TILES_MANHATTAN alternates 0 / 1 call by call (0 launches what a library without the switch launches, so it is the
baseline), every query set warmed up at both settings first, `--calls` timed calls a setting.  Per query set and setting: p50 /
p99 / min / max of the wall clock of the call (Python wrapper included) and the ah_search_stats of the timed calls.  Query sets:
`distinct` — one query near each of 1000 items, leaves mostly visited by one query; `clustered` — 16 queries near each of 63
items, so units of 9 - 16 visits, where the tile is bound by its VALU operations.

    timeout 900 python scripts/measure_manhattan_tiles.py [--shape 1000000,768,20] [--out profiles/manhattan_tiles.json]
    rocprofv3 --kernel-trace --stats -- python scripts/measure_manhattan_tiles.py --calls 5   (kernel time, a run of its own)
"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))

from arroy_amd import Dataset, _lib, shard  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

STATS = ("rerank_tiles", "rerank_sorted", "fallback_chunks", "tile_units_16", "tile_units_8", "tile_units_4", "tile_visits")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1000000,768,20", help="n,dims,trees")
    ap.add_argument("--count", type=int, default=100)
    ap.add_argument("--search-k", type=int, default=10_000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=21, help="timed calls a setting")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls a setting and query set")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, dims, trees = (int(x) for x in a.shape.split(","))
    ds = Dataset(D.Manhattan, dims, n)
    ds.fill_synthetic(42, 1, n)
    ds.finalize()
    forest = ds.build_forest(shard.tree_seeds(42, range(trees)))
    index = ds.create_index(forest)
    rng = np.random.default_rng(5)
    noise = rng.standard_normal((a.nq, dims)).astype(np.float32) * np.float32(0.05)
    rows = _lib.synth_rows_host(42, 1, a.nq, dims, first_item=0)
    sets = {"distinct": np.ascontiguousarray(rows + noise, dtype=np.float32),
            "clustered": np.ascontiguousarray(rows[np.arange(a.nq) // 16] + noise * np.float32(0.02), dtype=np.float32)}
    out = {"shape": a.shape, "count": a.count, "search_k": a.search_k, "nq": a.nq, "calls": a.calls, "sets": {}}
    answers = {}
    for name, queries in sets.items():
        t, stats = {0: [], 1: []}, {0: dict.fromkeys(STATS, 0), 1: dict.fromkeys(STATS, 0)}
        for rep in range(2 * (a.warmup + a.calls)):
            on = rep & 1
            index.stats(reset=True)
            with _lib.tuning(AH_SEARCH_TILES_MANHATTAN=on):
                t0 = time.perf_counter()
                got = index.search(a.count, queries=queries, search_k=a.search_k, raw=True)
                dt = time.perf_counter() - t0
            if rep >= 2 * a.warmup:
                t[on].append(dt)
                st = index.stats()
                for k in STATS:
                    stats[on][k] += int(st[k])
            if rep < 2:  # the two settings answer alike: ids, distance bits, counts
                answers[on] = got
        assert all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
                   for x, y in zip(answers[0], answers[1])), f"{name}: the settings answer differently"
        out["sets"][name] = {}
        for on in (0, 1):
            print(f"{name:10s} switch {on}: ah_search_stats of its {a.calls} timed calls: " + ", ".join(f"{k} {v}" for k, v in stats[on].items()), flush=True)
            p50, p99 = np.percentile(t[on], [50, 99])
            out["sets"][name][f"switch {on}"] = {"p50_s": p50, "p99_s": p99, "min_s": min(t[on]), "max_s": max(t[on]), "calls": len(t[on]),
                                                  "qps": a.nq / p50, "stats_of_timed_calls": stats[on]}
            print(f"{name:10s} switch {on}: p50 {1e3 * p50:8.3f} ms  p99 {1e3 * p99:8.3f}  min {1e3 * min(t[on]):8.3f}  max {1e3 * max(t[on]):8.3f}  "
                  f"({a.nq / p50:9.0f} queries/s)", flush=True)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    index.close()
    forest.close()
    ds.close()


if __name__ == "__main__":
    main()
