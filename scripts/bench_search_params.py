#!/usr/bin/env python3
"""Per-query search parameters in one call against one call per parameter set: what DESIGN.md §4 "Per-query search parameters"
reports.

One process, the benchmark's search index (1M x 1536 dot product, 20 trees), 1000 queries that start from distinct items, 8
(count, search_k, oversampling) sets spread unevenly over the queries.  Timed, alternating in one process after a warm-up of
every shape, each until its window is a second or more:
  (a) ah_search_batch_params, one call;
  (b) the same queries as one ah_search_batch call per parameter set — what a host does without the entry point;
  (b') (b) once more, interleaved the same way: its own run-to-run spread;
  (c) equal params: ah_search_batch_params against ah_search_batch_filters with the same scalars.
The outputs of (a) and (b) are compared for bit equality.  Prints one JSON line.

    timeout -k 10 600 python scripts/bench_search_params.py [--drop-sets 5] [--out profiles/search_params.json]
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
# (count, search_k, oversampling, share of the queries): limit + offset as count, search_k raised for paginated or re-ranked requests
SETS = [(20, 0, 0, 0.34), (100, 10_000, 0, 0.25), (10, 2_000, 0, 0.15), (50, 0, 2, 0.10), (200, 20_000, 0, 0.07), (1000, 0, 0, 0.05),
        (100, 50_000, 0, 0.03), (3000, 0, 0, 0.01)]


def alternate(legs, window):
    """Every leg in turn, round after round, until each has run for `window` seconds: {name: [seconds per run]}."""
    times = {name: [] for name, _ in legs}
    while min(sum(t) for t in times.values()) < window:
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1000000,1536,20,dot", help="n,dims,trees,metric")
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--window", type=float, default=1.5, help="seconds of timed runs per leg at the least")
    ap.add_argument("--drop-sets", default="", help="comma list of positions in SETS to leave out (e.g. 5: the count at the selection's capacity)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    global SETS
    SETS = [s for i, s in enumerate(SETS) if str(i) not in a.drop_sets.split(",")]
    n, dims, trees, metric = a.shape.split(",")
    n, dims, trees = int(n), int(dims), int(trees)
    ds = Dataset(METRICS[metric], dims, n)
    ds.fill_synthetic(42, 1, n)
    if metric == "dot":
        ds.preprocess_dot()
    ds.finalize()
    forest = ds.build_forest(shard.tree_seeds(42, range(trees)))
    index = ds.create_index(forest)
    rng = np.random.default_rng(5)
    nq = a.nq
    queries = np.stack([ds.item_vector(int(i)) for i in rng.choice(n, nq, replace=False)])
    queries = np.ascontiguousarray(queries + rng.standard_normal((nq, dims)).astype(np.float32) * np.float32(0.05), dtype=np.float32)
    share = np.array([s[3] for s in SETS])
    set_of = rng.choice(len(SETS), nq, p=share / share.sum())
    set_of[:len(SETS)] = np.arange(len(SETS))  # every set at least once
    counts = np.array([SETS[s][0] for s in set_of], dtype=np.int64)
    sks = np.array([SETS[s][1] for s in set_of], dtype=np.int64)
    overs = np.array([SETS[s][2] for s in set_of], dtype=np.int64)
    groups = [np.flatnonzero(set_of == s) for s in range(len(SETS))]
    qs_of = [np.ascontiguousarray(queries[g]) for g in groups]

    def one_call():
        return index.search_params(counts, queries=queries, search_ks=sks, oversamplings=overs, raw=True)

    def per_set():
        return [index.search(SETS[s][0], queries=qs_of[s], search_k=SETS[s][1], oversampling=SETS[s][2], raw=True) for s in range(len(SETS))]

    # bit equality of the two ways, and the warm-up of every shape
    index.params_stats(reset=True)
    index.stats(reset=True)
    got, want = one_call(), per_set()
    pst, sst = index.params_stats(), index.stats()
    equal = True
    for s, g in enumerate(groups):
        c = SETS[s][0]
        equal = equal and np.array_equal(got[2][g], want[s][2]) and np.array_equal(got[0][g, :c], want[s][0])
        equal = equal and np.array_equal(got[1][g, :c].view(np.uint32), want[s][1].view(np.uint32))
        equal = equal and bool((got[0][g, c:] == 0xFFFFFFFF).all())
    c0, sk0 = 100, 10_000

    def equal_params():
        return index.search_params(c0, queries=queries, search_ks=sk0, raw=True)

    def filters_entry():
        return index.search(c0, queries=queries, search_k=sk0, filters=[], raw=True)

    for fn in (one_call, per_set, equal_params, filters_entry):
        fn()
    t = alternate([("a one ah_search_batch_params call", one_call), ("b one ah_search_batch call per set", per_set),
                   ("b' the same once more", per_set)], a.window)
    t.update(alternate([("c equal params: ah_search_batch_params", equal_params), ("c equal params: ah_search_batch_filters", filters_entry),
                        ("c' ah_search_batch_filters once more", filters_entry)], a.window))
    out = {"shape": a.shape, "nq": nq, "sets": [{"count": s[0], "search_k": s[1], "oversampling": s[2], "queries": int(g.size)}
                                                for s, g in zip(SETS, groups)],
           "bit_equal": bool(equal), "params_stats": pst, "search_stats_of_both_ways": {k: v for k, v in sst.items() if v}, "legs": {}}
    for name, sec in t.items():
        med = statistics.median(sec)
        out["legs"][name] = {"runs": len(sec), "median_ms": 1e3 * med, "min_ms": 1e3 * min(sec), "max_ms": 1e3 * max(sec),
                             "us_per_query": 1e6 * med / nq}
        print(f"{name:44s} {1e3 * med:9.3f} ms  ({1e6 * med / nq:7.2f} us per query; min {1e3 * min(sec):.3f} max {1e3 * max(sec):.3f}; {len(sec)} runs)",
              flush=True)
    print(f"bit equal: {equal}; params stats: {pst}", flush=True)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    index.close()
    forest.close()
    ds.close()
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
