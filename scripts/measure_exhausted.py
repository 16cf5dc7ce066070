#!/usr/bin/env python3
"""Exhausted filters (AH_SEARCH_EXHAUSTED) against the descent they replace: what DESIGN.md §4 "Exhausted filters" reports.

One process, one index (default 1M x 768 cosine, 20 trees, synthetic rows), resident filters of 100 and 1000 stored ids,
search_k = 10 000, calls of 1, 64 and 1000 queries that start from distinct items.  For every (filter, call size) the tunable is
set to 0 and 1 alternately — 0 IS the path without the feature — after a warm-up of both; each leg runs at least `--runs`
times unless its runs already add up to `--cap` seconds (never fewer than 3).  The two outputs are compared bit for bit.  A
filter whose kept_total exceeds the effective search_k is not exhausted: both legs then take the same path, and the line says
so.  The first use of a filter (kept_total + the kept list) is timed on its own, on fresh filters.  Prints one JSON line per
case and a summary line.

    timeout -k 10 900 python scripts/measure_exhausted.py [--shape 1000000,768,20,cosine] [--out profiles/exhausted.json]
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))

from arroy_amd import Dataset, _lib, shard  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

METRICS = {"cosine": D.Cosine, "dot": D.DotProduct, "euclidean": D.Euclidean}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1000000,768,20,cosine", help="n,dims,trees,metric")
    ap.add_argument("--filters", default="100,1000", help="stored ids of the filters")
    ap.add_argument("--calls", default="1,64,1000", help="queries per call")
    ap.add_argument("--search-k", default="10000", help="comma list; every filter is measured at each")
    ap.add_argument("--count", type=int, default=10)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--cap", type=float, default=25.0, help="seconds of timed runs per leg at the most (at least 3 runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, dims, trees, metric = a.shape.split(",")
    n, dims, trees = int(n), int(dims), int(trees)
    t0 = time.perf_counter()
    ds = Dataset(METRICS[metric], dims, n)
    ds.fill_synthetic(42, 1, n)
    if metric == "dot":
        ds.preprocess_dot()
    ds.finalize()
    forest = ds.build_forest(shard.tree_seeds(42, range(trees)))
    index = ds.create_index(forest)
    setup = time.perf_counter() - t0
    rng = np.random.default_rng(1)
    max_nq = max(int(c) for c in a.calls.split(","))
    items = rng.choice(n, max_nq, replace=False).astype(np.uint32)
    lines = []
    try:
        for n_ids in (int(x) for x in a.filters.split(",")):
            ids = np.sort(rng.choice(n, n_ids, replace=False)).astype(np.uint32)
            # first use, on fresh filters: kept_total alone, then the list (tunable on, one query), against the same call afterwards
            first = {"kept_total_ms": [], "list_ms": []}
            for _ in range(5):
                f = index.make_filter(ids, sorted=True)
                t = time.perf_counter()
                total = f.kept_total()
                first["kept_total_ms"].append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter()
                m = f.kept_ids().size
                first["list_ms"].append((time.perf_counter() - t) * 1e3)
                f.close()
            f = index.make_filter(ids, sorted=True)
            for sk in (int(x) for x in a.search_k.split(",")):
                for nq in (int(c) for c in a.calls.split(",")):
                    kw = dict(items=items[:nq], search_k=sk, raw=True, filters=[f])
                    out, times = {}, {0: [], 1: []}
                    for on in (0, 1):  # warm-up of both legs, and the outputs
                        with _lib.tuning(AH_SEARCH_EXHAUSTED=on):
                            out[on] = index.search(a.count, **kw)
                    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(out[0], out[1])), "the two legs differ"
                    index.exhausted_stats(reset=True)
                    while any(len(times[on]) < 3 or (len(times[on]) < a.runs and sum(times[on]) < a.cap) for on in (0, 1)):
                        for on in (0, 1):
                            with _lib.tuning(AH_SEARCH_EXHAUSTED=on):
                                t = time.perf_counter()
                                index.search(a.count, **kw)  # (returns after its last copy has landed)
                                times[on].append(time.perf_counter() - t)
                    xs = index.exhausted_stats()
                    line = {"filter_ids": n_ids, "kept_total": total, "list_ids": int(m), "search_k": sk, "queries": nq, "count": a.count,
                            "exhausted": bool(xs["queries"] > 0), "runs": len(times[0]),
                            "off_ms_median": statistics.median(times[0]) * 1e3, "on_ms_median": statistics.median(times[1]) * 1e3,
                            "off_ms_min_max": [min(times[0]) * 1e3, max(times[0]) * 1e3],
                            "on_ms_min_max": [min(times[1]) * 1e3, max(times[1]) * 1e3],
                            "first_use_kept_total_ms_median": statistics.median(first["kept_total_ms"]),
                            "first_use_list_ms_median": statistics.median(first["list_ms"]), "bit_equal": True}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
            f.close()
    finally:
        index.close()
        forest.close()
        ds.close()
    summary = {"shape": a.shape, "setup_seconds": setup, "device": __import__("arroy_amd").device_name(0), "cases": lines}
    print(json.dumps(summary))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(summary, fh, indent=1)


if __name__ == "__main__":
    main()
