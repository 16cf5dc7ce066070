#!/usr/bin/env python3
"""The build-to-index hand-over, host view against resident forest: what DESIGN.md §4 "Resident forests" reports.

One process per shape (`--shape n,dims,trees`, Cosine, synthetic rows), after one warm-up of every leg, `--reps` repetitions
(>= 5), medians of wall time:
  (a) ah_build_forest + ah_index_create + the first ah_search_batch (16 queries);
  (b) ah_build_forest_resident + ah_index_create_from_forest + the first search;
  (c) the extra device time of the resident stage: its own HIP-event time, which ah_forest_stats counts in seconds_device and
      the library prints per batch under AH_TIMING — read from three further resident builds run with AH_TIMING=1 (outside
      the timed repetitions: the switch makes a build wait after its phases), summed over the batches of each build; the
      difference of the medians of seconds_device of (b) and (a) is reported next to it, and is within their spread;
and the same pair for a sub-tree build of `--lists` id lists (leaves of a one-tree forest built with split_after n / lists,
re-split with split_after 64) grafted onto the index of that forest: ah_build_subtrees + ah_index_graft against the _resident build + ah_index_graft_forest.
`--plain-only LIB` times only ah_build_forest, with the library at LIB (a build of the parent commit): the wall time of the
non-resident build before and after this change, measured the same way; the caller merges both into one file.

    python scripts/exp_forest_resident.py --shape 10000000,768,100 --reps 5 --out profiles/exp_forest_resident.json
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arroy_amd import _lib  # noqa: E402

NEW = ("ah_build_forest_resident", "ah_build_subtrees_resident", "ah_forest_resident_info", "ah_forest_release_device",
       "ah_index_create_from_forest", "ah_index_graft_forest")


def med(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1000000,768,50", help="n,dims,trees")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lists", type=int, default=4096)
    ap.add_argument("--plain-only", default=None, help="time ah_build_forest only, with this library")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.plain_only:
        _lib.LIB_PATH = os.path.abspath(a.plain_only)
        probe = __import__("ctypes").CDLL(_lib.LIB_PATH)
        for name in NEW:
            if not hasattr(probe, name):
                _lib.SIGNATURES.pop(name, None)
    from arroy_amd import Dataset, Index, shard
    from arroy_amd import distances as D
    n, dims, trees = (int(x) for x in a.shape.split(","))
    ds = Dataset(D.Cosine, dims, n)
    ds.fill_synthetic(42, 1, n)
    ds.finalize()
    seeds = shard.tree_seeds(42, range(trees))
    queries = np.random.default_rng(1).standard_normal((16, dims)).astype(np.float32)
    out = {"shape": a.shape, "reps": a.reps, "library": a.plain_only or "this commit"}

    def hand_over(resident):
        t0 = time.perf_counter()
        forest = ds.build_forest(seeds, resident=True) if resident else ds.build_forest(seeds)
        t1 = time.perf_counter()
        ix = Index.from_forest(ds, forest) if resident else Index(ds, forest)
        t2 = time.perf_counter()
        res = ix.search(10, queries=queries, raw=True)
        t3 = time.perf_counter()
        assert not resident or ix.from_device
        row = {"build": t1 - t0, "index": t2 - t1, "search": t3 - t2, "total": t3 - t0, "device": forest.stats["seconds_device"],
               "digest": forest.digest()[0] if n <= 1_000_000 else 0, "answer": res[0].tobytes()}
        ix.close()
        forest.close()
        return row

    def stage_seconds():
        """one resident build under AH_TIMING with stderr captured: the stage's device time, summed over its batches"""
        with tempfile.TemporaryFile() as tmp:
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                with _lib.tuning(AH_TIMING=1):
                    ds.build_forest(seeds, resident=True).close()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            ms = re.findall(r"resident stage: .*?: ([0-9.]+) ms on the device", tmp.read().decode(errors="replace"))
        assert ms, "the library printed no resident stage"
        return sum(float(x) for x in ms) * 1e-3

    if a.plain_only:
        t = []
        for _rep in range(a.reps + 1):
            t0 = time.perf_counter()
            forest = ds.build_forest(seeds)
            t.append(time.perf_counter() - t0)
            forest.close()
        out["build_forest"] = med(t[1:])
    else:
        rows = {False: [], True: []}
        for rep in range(a.reps + 1):
            for resident in (False, True):
                rows[resident].append(hand_over(resident))
        assert rows[False][0]["answer"] == rows[True][0]["answer"] and rows[False][0]["digest"] == rows[True][0]["digest"]
        for resident, name in ((False, "a_host_view"), (True, "b_resident")):
            out[name] = {k: med([r[k] for r in rows[resident][1:]]) for k in ("build", "index", "search", "total", "device")}
        out["build_forest"] = out["a_host_view"]["build"]
        out["c_stage_device"] = med([stage_seconds() for _ in range(3)])
        out["c_seconds_device_difference_s"] = out["b_resident"]["device"]["median_s"] - out["a_host_view"]["device"]["median_s"]
        # the sub-tree leg: leaves of a one-tree forest cut at n / lists items, re-split at 64
        sub_split = 64
        base = ds.build_forest(seeds[:1], split_after=max(2 * sub_split + 2, n // a.lists))
        leaves = [i for i in np.flatnonzero(base.nodes["kind"] == 1) if base.nodes["count"][i] > sub_split][:a.lists]
        lists = [np.sort(base.descendants[int(base.nodes["offset"][i]):int(base.nodes["offset"][i]) + int(base.nodes["count"][i])])
                 for i in leaves]
        targets = np.array(leaves, dtype=np.uint32)
        sub_seeds = shard.tree_seeds(7, range(len(lists)))
        sub = {False: [], True: []}
        for rep in range(a.reps + 1):
            for resident in (False, True):
                ix = Index(ds, base)
                t0 = time.perf_counter()
                f = ds.build_subtrees(lists, sub_seeds, split_after=sub_split, resident=resident)
                t1 = time.perf_counter()
                if resident:
                    assert ix.graft_forest(f, targets)
                else:
                    ix.graft(f.view_struct(), targets)
                t2 = time.perf_counter()
                sub[resident].append({"build": t1 - t0, "graft": t2 - t1, "total": t2 - t0, "device": f.stats["seconds_device"]})
                ix.close()
                f.close()
        assert len(lists) > 0
        out["subtrees"] = {"lists": len(lists), "ids": int(sum(len(x) for x in lists)), "split_after": sub_split}
        for resident, name in ((False, "a_host_view"), (True, "b_resident")):
            out["subtrees"][name] = {k: med([r[k] for r in sub[resident][1:]]) for k in ("build", "graft", "total", "device")}
        base.close()
    print(json.dumps(out), flush=True)
    if a.out:
        prev = json.load(open(a.out)) if os.path.exists(a.out) else {}
        prev.setdefault(a.shape, {})["parent_commit" if a.plain_only else "this_commit"] = out
        json.dump(prev, open(a.out, "w"), indent=1)
        open(a.out, "a").write("\n")
    ds.close()


if __name__ == "__main__":
    main()
