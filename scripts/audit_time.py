#!/usr/bin/env python3
"""Auditing a resident index on the device against exporting it: what DESIGN.md §4 "Audit of a resident index" reports.

A narrow dataset (only the ids matter: 8 dimensions), `--trees` trees.  Seconds, median of `--reps` repetitions after one warm-up:
  (a) ah_index_audit with the per-tree stats, under AH_AUDIT_COVER_MB = 0 (one tree a pass) and under its default;
  (b) Index.export(normals=False): every node and every descendant id to the host;
  (c) (b) plus a numpy check of the export on the host (`host_check`: the class definitions of the audit, vectorised, for a
      structure that is a forest) — the only means there was before.

    timeout -k 10 300 python scripts/audit_time.py [--rows 10000000 --trees 20] [--out profiles/index_audit.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arroy_amd import Dataset, Index, _lib, shard  # noqa: E402
from arroy_amd import distances as D  # noqa: E402


def host_check(ex, stored_ids):
    """valid, floating, unsorted, foreign, duplicate, missing of an export whose reachable structure is a forest"""
    nodes, roots, desc = ex["nodes"], ex["roots"], ex["descendants"]
    kind, n_trees = nodes["kind"], len(roots)
    owner = np.zeros(len(nodes), dtype=np.int32)
    frontier = roots.astype(np.int64)
    owner[frontier] = np.arange(1, n_trees + 1)
    while frontier.size:
        split = frontier[kind[frontier] == 2]
        kids = np.concatenate([nodes["left"][split], nodes["right"][split]]).astype(np.int64)
        assert (owner[kids] == 0).all(), "a node is linked twice: not a forest"
        owner[kids] = np.concatenate([owner[split], owner[split]])
        frontier = kids
    floating = int(((kind != 0) & (owner == 0)).sum())
    leaves = np.flatnonzero((kind == 1) & (owner != 0))
    off, cnt = nodes["offset"][leaves].astype(np.int64), nodes["count"][leaves].astype(np.int64)
    start = np.cumsum(cnt) - cnt
    ids = desc if (off == start).all() and cnt.sum() == desc.size else desc[np.repeat(off - start, cnt) + np.arange(cnt.sum())]
    rising = ids[1:] > ids[:-1]
    rising[start[(start > 0) & (start < ids.size)] - 1] = True  # (the first id of a list has no neighbour)
    broken_at = np.flatnonzero(~rising) + 1
    unsorted = int(np.unique(np.searchsorted(start, broken_at, side="right")).size)
    if stored_ids.size and int(stored_ids[-1]) == stored_ids.size - 1:  # ids 0 .. n - 1 (ascending and distinct): the row is the id
        rows = ids.astype(np.int64)
        stored = rows < stored_ids.size
    else:
        rows = np.searchsorted(stored_ids, ids)
        stored = (rows < stored_ids.size) & (stored_ids[np.minimum(rows, stored_ids.size - 1)] == ids)
    foreign = int((~stored).sum())
    tree = np.repeat(owner[leaves].astype(np.int64) - 1, cnt)
    seen = np.bincount(tree[stored] * stored_ids.size + rows[stored], minlength=n_trees * stored_ids.size)
    duplicate, missing = int((seen[seen > 1] - 1).sum()), int((seen == 0).sum())
    return {"valid": int(not (floating or unsorted or foreign or duplicate or missing)), "floating": floating, "unsorted": unsorted,
            "foreign": foreign, "duplicate": duplicate, "missing": missing}


class Lines:
    """every line goes to stdout and to the file as soon as it is known"""

    def __init__(self, path):
        self.f = None
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            self.f = open(path, "w")

    def append(self, line):
        print(line, flush=True)
        if self.f:
            self.f.write(line + "\n")
            self.f.flush()

    def __iadd__(self, lines):
        for line in lines:
            self.append(line)
        return self


def timed(fn, reps):
    t = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        res = fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t[1:]), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--split-after", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = 8
    t0 = time.perf_counter()
    ds = Dataset(D.Euclidean, dims, a.rows)
    ds.fill_synthetic(42, 1, a.rows)
    ds.finalize()
    forest = ds.build_forest(shard.tree_seeds(42, range(a.trees)), split_after=a.split_after)
    print(f"staged and built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    ix = Index(ds, None, view=forest.view_struct())
    print(f"index after {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    info = ix.export_info()
    stored = np.arange(a.rows, dtype=np.uint32)
    lines = Lines(a.out)
    lines += [f"# python scripts/audit_time.py --rows {a.rows} --trees {a.trees} --split-after {a.split_after} --reps {a.reps}",
             f"# {_lib.device_name(0)}: {a.rows} rows x {dims} dims, {a.trees} trees, {info['n_nodes']} nodes, {info['desc_len']} ids "
             f"({info['desc_len'] * 4 / 1e6:.0f} MB); seconds, median of {a.reps} after one warm-up"]
    reports = []
    for mb in (0, None):
        with _lib.tuning(**({} if mb is None else {"AH_AUDIT_COVER_MB": mb})):
            s, r = timed(lambda: ix.audit(trees=True), a.reps)
        reports.append(r)
        lines.append(f"(a) ah_index_audit, AH_AUDIT_COVER_MB={_lib.tuning_get('AH_AUDIT_COVER_MB')[1] if mb is None else mb}: {s:.4f} s"
                     f"  (valid {r['valid']}, {r['nodes_reached']} nodes reached)")
    assert reports[0] == reports[1] and reports[0]["valid"] == 1
    s, ex = timed(lambda: ix.export(normals=False), a.reps)
    lines.append(f"(b) Index.export(normals=False): {s:.4f} s")
    s, chk = timed(lambda: host_check(ix.export(normals=False), stored), a.reps)
    lines.append(f"(c) (b) + numpy check of the export on the host: {s:.4f} s  (valid {chk['valid']})")
    assert chk["valid"] == 1
    ix.close()
    forest.close()
    ds.close()


if __name__ == "__main__":
    main()
