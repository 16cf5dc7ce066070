#!/usr/bin/env python3
"""Filtered search with and without resident filters: what DESIGN.md §4 "Resident candidate filters" reports.

One process, one index.  Legs (queries/s or ms per call, median of `--reps` timed repetitions after a warm-up):
  (a) one filtered query per call at stored shares 0.5 and 0.05: ah_search_batch with the id list, against a resident filter;
  (b) 1000 queries over 8 filters: one ah_search_batch call per filter, against one ah_search_batch_filters call;
  (c) 1000 queries, each under one of 64 filters: 64 calls against one call, the latter swept over AH_SEARCH_FILTER_GROUP_MIN;
  (d) the unfiltered 1000-query call;
  (e) one composite filter a AND b (shares 0.5 x 0.5 and 0.5 x 0.01) made three ways, each alone and with the one-query search
      that follows: the host's list of the result through ah_filter_create, the host's bitmap through ah_filter_create_bitmap,
      ah_filter_combine of the two resident operands.  A library without the last two runs the list way only.
A library without ah_filter_create (the parent commit) runs the per-list legs only, so the same script measures both trees:
run them alternating, three runs each, and compare every run of one with every run of the other.

    timeout 900 python scripts/measure_filters.py --shape 1000000,1536,20,dot [--out profiles/filters_<tree>_<run>.json]
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


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1000000,1536,20,dot", help="n,dims,trees,metric")
    ap.add_argument("--count", type=int, default=100)
    ap.add_argument("--search-k", type=int, default=10_000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep", default="1,4,8,16,32,64,100000")
    ap.add_argument("--legs", default="abcde", help="which legs to run, e.g. 'e' for the composite-filter leg alone")
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
    resident = hasattr(_lib.lib(), "ah_filter_create") and hasattr(index, "make_filter")
    rng = np.random.default_rng(5)
    queries = _lib.synth_rows_host(42, 1, a.nq, dims, first_item=0) + rng.standard_normal((a.nq, dims)).astype(np.float32) * np.float32(0.05)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    ids = np.arange(n, dtype=np.uint32)
    kw = dict(search_k=a.search_k, raw=True)
    out = {"shape": a.shape, "count": a.count, "search_k": a.search_k, "nq": a.nq, "resident_filters": resident, "legs": {}}

    def note(name, sec, per):
        med, lo, hi = sec
        out["legs"][name] = {"median_s": med, "min_s": lo, "max_s": hi, "per": per,
                             "qps": per / med, "ms_per_call": 1e3 * med}
        print(f"{name:48s} {1e3 * med:9.3f} ms  ({per / med:10.0f} queries/s; min {1e3 * lo:.3f} max {1e3 * hi:.3f})", flush=True)

    # (a) one filtered query per call
    for share in (0.5, 0.05) if "a" in a.legs else ():
        lst = ids[::int(round(1 / share))].copy()
        one = queries[:1]
        note(f"a share {share}: list per call", timed(lambda: index.search(a.count, queries=one, candidates=lst, candidates_sorted=True, **kw), 20 * a.reps), 1)
        if resident:
            with index.make_filter(lst, sorted=True) as f:
                note(f"a share {share}: resident filter", timed(lambda: index.search(a.count, queries=one, filters=[f], **kw), 20 * a.reps), 1)
    # (b), (c): nq queries over 8 / 64 filters of mixed shares
    for name, n_filters in [x for x in (("b", 8), ("c", 64)) if x[0] in a.legs]:
        steps = [2, 3, 5, 10, 20, 40, 100, 7]
        lists = [ids[(i % 3)::steps[i % len(steps)] + i // len(steps)].copy() for i in range(n_filters)]
        slots = rng.integers(0, n_filters, a.nq).astype(np.uint32)
        groups = [np.flatnonzero(slots == s) for s in range(n_filters)]
        qs_of = [np.ascontiguousarray(queries[g]) for g in groups]

        def per_list():
            for s in range(n_filters):
                if groups[s].size:
                    index.search(a.count, queries=qs_of[s], candidates=lists[s], candidates_sorted=True, **kw)
        note(f"{name} {n_filters} filters: one list call per filter", timed(per_list, a.reps), a.nq)
        if resident:
            filters = [index.make_filter(x, sorted=True) for x in lists]
            for gmin in [int(x) for x in a.sweep.split(",")]:
                with _lib.tuning(AH_SEARCH_FILTER_GROUP_MIN=gmin):
                    note(f"{name} {n_filters} filters: one call, group min {gmin}",
                         timed(lambda: index.search(a.count, queries=queries, filters=filters, filter_of_query=slots, **kw), a.reps), a.nq)
            note(f"{name} {n_filters} filters: one call, default group min",
                 timed(lambda: index.search(a.count, queries=queries, filters=filters, filter_of_query=slots, **kw), a.reps), a.nq)
            for f in filters:
                f.close()
    # (e) the same composite filter a AND b made three ways, alone and with the one-query search that follows: the expression
    # evaluated by numpy and uploaded as a list, the host's bitmap of it, and ah_filter_combine of the two resident operands
    combine = resident and hasattr(_lib.lib(), "ah_filter_combine") and hasattr(index, "combine_filters")
    out["combine"] = bool(combine)
    one = queries[:1]
    for share_a, share_b in ((0.5, 0.5), (0.5, 0.01)) if "e" in a.legs else ():
        tag = f"e {share_a} x {share_b}"
        list_a = np.sort(rng.choice(n, int(n * share_a), replace=False)).astype(np.uint32)
        list_b = np.sort(rng.choice(n, int(n * share_b), replace=False)).astype(np.uint32)
        # what the host holds: one bitmap per operand (the stored facets); the expression itself is a word-wise AND of them
        bits_a, bits_b = np.zeros((n + 63) // 64 * 64, np.bool_), np.zeros((n + 63) // 64 * 64, np.bool_)
        bits_a[list_a], bits_b[list_b] = True, True
        words_a = np.packbits(bits_a, bitorder="little").view(np.uint64)
        words_b = np.packbits(bits_b, bitorder="little").view(np.uint64)

        def host_list():  # evaluate, then walk the result into the ascending id list
            return np.flatnonzero(np.unpackbits((words_a & words_b).view(np.uint8), bitorder="little")).astype(np.uint32)

        def search_under(f):
            index.search(a.count, queries=one, filters=[f], **kw)
            f.close()

        note(f"{tag}: list per call + query", timed(lambda: index.search(a.count, queries=one, candidates=host_list(), candidates_sorted=True, **kw), 5 * a.reps), 1)
        if resident:
            note(f"{tag}: list -> ah_filter_create", timed(lambda: index.make_filter(host_list(), sorted=True).close(), 5 * a.reps), 1)
            note(f"{tag}: list -> ah_filter_create + query", timed(lambda: search_under(index.make_filter(host_list(), sorted=True)), 5 * a.reps), 1)
        if combine:
            note(f"{tag}: bitmap -> ah_filter_create_bitmap", timed(lambda: index.make_filter_bitmap(words_a & words_b, n).close(), 5 * a.reps), 1)
            note(f"{tag}: bitmap -> ah_filter_create_bitmap + query", timed(lambda: search_under(index.make_filter_bitmap(words_a & words_b, n)), 5 * a.reps), 1)
            with index.make_filter(list_a, sorted=True) as fa, index.make_filter(list_b, sorted=True) as fb:
                note(f"{tag}: ah_filter_combine of two resident", timed(lambda: (fa & fb).close(), 5 * a.reps), 1)
                note(f"{tag}: ah_filter_combine of two resident + query", timed(lambda: search_under(fa & fb), 5 * a.reps), 1)
                with _lib.tuning(AH_FILTER_COMBINE_SHORTCUT=0):
                    note(f"{tag}: ah_filter_combine, every leaf walked", timed(lambda: (fa & fb).close(), 5 * a.reps), 1)
    # (d) unfiltered
    if "d" in a.legs:
        note("d unfiltered ah_search_batch", timed(lambda: index.search(a.count, queries=queries, **kw), a.reps), a.nq)
    if "d" in a.legs and resident:
        note("d unfiltered ah_search_batch_filters", timed(lambda: index.search(a.count, queries=queries, filters=[], **kw), a.reps), a.nq)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    index.close()
    forest.close()
    ds.close()


if __name__ == "__main__":
    main()
