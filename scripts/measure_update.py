"""Cost of updating a staged dataset against staging it afresh: 10M x 768 Cosine on one device.

Prints the medians of
  * ah_dataset_update_vectors with 1k, 10k and 100k changes (a third removed ids, a third replaced rows, a third new ids);
  * staging the dataset from scratch (ah_dataset_upload_vectors in 1M-row calls + ah_dataset_finalize; the host rows are
    generated outside the timed calls);
  * the first full scan and the first 10-tree build after an update (they rebuild the packed / binary16 / int8 copies),
    next to the same calls once the copies exist.

    python scripts/measure_update.py [--n 10000000] [--dims 768] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arroy_amd import Dataset, _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    n, dims = args.n, args.dims
    out = {"n": n, "dims": dims}

    # staging from scratch
    chunk = 1_000_000
    host = np.empty((min(chunk, n), dims), dtype=np.float32)
    stage = []
    for _ in range(args.reps):
        ds = Dataset(D.Cosine, dims, n)
        spent = 0.0
        for lo in range(0, n, chunk):
            c = min(chunk, n - lo)
            _lib.synth_rows_host(42, 1, c, dims, first_item=lo, out=host[:c])
            t = time.perf_counter()
            ds.upload_vectors(np.arange(lo, lo + c, dtype=np.uint32), host[:c])
            spent += time.perf_counter() - t
        t = time.perf_counter()
        ds.finalize()
        stage.append(spent + time.perf_counter() - t)
        ds.close()
    out["stage_s"] = med(stage)

    # updates of a dataset filled on the device (ids 0 .. n-1)
    rng = np.random.default_rng(1)
    ds = Dataset(D.Cosine, dims, n)
    ds.fill_synthetic(42, 1, n)
    ds.finalize()
    present = np.arange(n, dtype=np.int64)
    next_id = n
    for k in (1_000, 10_000, 100_000):
        times = []
        for _ in range(args.reps):
            third = k // 3
            pick = rng.choice(present.size, 2 * third, replace=False)
            removed, replaced = np.sort(present[pick[:third]]), np.sort(present[pick[third:]])
            new = np.arange(next_id, next_id + (k - 2 * third), dtype=np.int64)
            next_id += new.size
            upsert = np.union1d(replaced, new).astype(np.uint32)
            vecs = rng.standard_normal((upsert.size, dims)).astype(np.float32)
            t = time.perf_counter()
            ds.update_vectors(removed.astype(np.uint32), upsert, vecs)
            times.append(time.perf_counter() - t)
            present = np.union1d(np.setdiff1d(present, removed), new)
        out[f"update_{k}_s"] = med(times)
    assert len(ds) == present.size

    # the first calls after an update rebuild the copies of the rows
    first_scan, scan, first_build, build = [], [], [], []
    seeds = list(range(1, 11))
    for _ in range(args.reps):
        ds.update_vectors(np.zeros(0, np.uint32), np.array([next_id], np.uint32), rng.standard_normal((1, dims)).astype(np.float32))
        next_id += 1
        q = int(present[0])
        for lst in (first_scan, scan):
            t = time.perf_counter()
            ds.distances(item=q)
            lst.append(time.perf_counter() - t)
        ds.update_vectors(np.zeros(0, np.uint32), np.array([next_id], np.uint32), rng.standard_normal((1, dims)).astype(np.float32))
        next_id += 1
        for lst in (first_build, build):
            t = time.perf_counter()
            ds.build_forest(seeds).close()
            lst.append(time.perf_counter() - t)
    out.update(first_scan_after_update_s=med(first_scan), scan_s=med(scan), first_build10_after_update_s=med(first_build),
               build10_s=med(build), update_paths=ds.update_paths())
    out["stage_over_update_10k"] = out["stage_s"] / out["update_10000_s"]
    ds.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
