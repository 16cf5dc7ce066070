#!/usr/bin/env python3
"""What keeping resident filters across index maintenance costs: DESIGN.md §4 "Filters across index maintenance".

One process, one index (default 1M x 768 Cosine, 20 trees), 64 filters that keep 1 .. 50 % of the ids.  Two ways to have the 64
filters valid again after a maintenance call, alternated rep by rep in the same run, host clock around calls that end in a
stream synchronise, median of `--reps` after a warm-up:
  (a) what a library without ah_filter_suspend offers: 64 x ah_filter_destroy + ah_filter_create from the host's ascending id
      lists (the lists are ready: the host's walk of its bitmaps into lists is timed apart, as (a-walk));
  (b) 64 x ah_filter_suspend + ONE ah_filter_resume_batch with 1000 edited ids per filter (500 removed, 500 added), also with
      AH_FILTER_RESUME_GROUP = 1 and 8 (a pass over the Descendants ids per filter / per 8 filters instead of per 16).
ah_filter_create is the same code as before the feature, so (a) is the baseline measured in the same run.  After the timed
part one resumed filter is compared bit for bit with the list-made filter of its set.

    python scripts/bench_filter_resume.py [--out profiles/filter_resume.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_filter_resume.py --profile --reps 3
(--profile: no timing; 3 x (a) and 3 x (b) at groups 1, 8 and 16, so that the kernel statistics hold k_leaf_kept next to
k_leaf_kept_group<1>, <8> and <16>: device time per pass = total / calls.)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arroy_amd import Dataset, _lib, shard  # noqa: E402
from arroy_amd import distances as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1000000,768,20", help="n,dims,trees")
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--edited", type=int, default=1000, help="edited ids per filter: half removed, half added")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, dims, trees = (int(x) for x in a.shape.split(","))
    ds = Dataset(D.Cosine, dims, n)
    ds.fill_synthetic(42, 1, n)
    ds.finalize()
    forest = ds.build_forest(shard.tree_seeds(42, range(trees)))
    index = ds.create_index(forest)
    info = index.export_info()
    rng = np.random.default_rng(7)
    shares = np.linspace(0.01, 0.5, a.filters)
    masks = [rng.random(n) < s for s in shares]
    lists = [np.flatnonzero(m).astype(np.uint32) for m in masks]
    half = a.edited // 2
    # the delta of every filter: `half` of its ids leave, `half` others join; every other rep applies it backwards
    fwd = [(np.sort(rng.choice(lst, half, replace=False)), np.sort(rng.choice(np.flatnonzero(~m).astype(np.uint32), half, replace=False)))
           for lst, m in zip(lists, masks)]
    back = [(add, rm) for rm, add in fwd]
    filters = [index.make_filter(x, sorted=True) for x in lists]
    state = {"flip": 0}

    def recreate():
        for i, f in enumerate(filters):
            f.close()
            filters[i] = index.make_filter(lists[i], sorted=True)
        state["flip"] = 0  # (the sets are the lists again)

    def resume(group):
        with _lib.tuning(AH_FILTER_RESUME_GROUP=group):
            for f in filters:
                f.suspend()
            st = index.resume_filters(filters, back if state["flip"] else fwd, want_stats=True, edits_sorted=True)
        state["flip"] ^= 1
        return st

    legs = [("a: 64 x destroy + create from lists", recreate), ("b: 64 x suspend + one resume_batch, group 16", lambda: resume(16)),
            ("b: group 8", lambda: resume(8)), ("b: group 1", lambda: resume(1))]
    if a.profile:
        for _name, fn in legs:
            for _ in range(a.reps):
                fn()
        print("profile run done", flush=True)
        return
    for _name, fn in legs:  # warm-up: every shape the timed window uses
        fn()
        fn()
    times = {name: [] for name, _ in legs}
    stats = None
    for _ in range(a.reps):  # the legs alternate: what else the host does meanwhile hits all of them alike
        for name, fn in legs:
            t0 = time.perf_counter()
            r = fn()
            times[name].append(time.perf_counter() - t0)
            if name.endswith("group 16"):
                stats = r
    t0 = time.perf_counter()
    walked = [np.flatnonzero(m).astype(np.uint32) for m in masks]
    walk_s = time.perf_counter() - t0
    assert all(np.array_equal(x, y) for x, y in zip(walked, lists))
    # faster and different is not faster: a resumed filter against the list-made filter of its set
    k = a.filters // 2
    want = lists[k] if state["flip"] == 0 else np.union1d(np.setdiff1d(lists[k], fwd[k][0]), fwd[k][1]).astype(np.uint32)
    with index.make_filter(want, sorted=True) as fresh:
        ge, we = filters[k].export(), fresh.export()
        same = bool(np.array_equal(ge["bits"], we["bits"]) and np.array_equal(ge["leaf_kept"], we["leaf_kept"])
                    and filters[k].info()["stored"] == fresh.info()["stored"])
    assert same, "a resumed filter differs from the list-made filter of its set"
    out = {"device": __import__("arroy_amd").device_name(0), "shape": a.shape, "filters": a.filters, "edited_per_filter": a.edited,
           "reps": a.reps, "n_nodes": info["n_nodes"], "desc_len": info["desc_len"], "resume_stats_group_16": stats,
           "walk_bitmaps_into_lists_ms": 1e3 * walk_s, "resumed_equals_list_made": same, "legs": {}}
    for name, _ in legs:
        t = times[name]
        out["legs"][name] = {"median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t)}
        print(f"{name:48s} {1e3 * statistics.median(t):9.3f} ms  (min {1e3 * min(t):.3f}, max {1e3 * max(t):.3f}; {a.filters} filters)", flush=True)
    print(f"{'a-walk: 64 host bitmaps into id lists (numpy)':48s} {1e3 * walk_s:9.3f} ms", flush=True)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    for f in filters:
        f.close()
    index.close()
    forest.close()
    ds.close()


if __name__ == "__main__":
    main()
