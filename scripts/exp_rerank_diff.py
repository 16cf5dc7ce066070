"""The difference screen of ah_rerank_batch (AH_RERANK_SCREEN_DIFF) on the configs[3] shape of
exp_rerank_batch.py — 1M x 1536 rows, 1000 queries x 10 000 - 11 535 sorted candidates, submissions of 125 queries from one
caller — for Euclidean and Manhattan rows, uniform and AH_SYNTH_CLUSTERED.  Settings 0 and 1 alternate in one process and the
answers are compared bit for bit.  A library that does not know the tunable (AH_LIB_PATH = a build of the parent commit) is
measured as it is, twice: the run-to-run spread the setting 0 has to stay within.  One JSON line per measurement."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arroy_amd import Dataset, distances, _lib  # noqa: E402

n, dims, nq, k = 1_000_000, 1536, 1000, 100
rng = np.random.default_rng(42)
lists = []
for _ in range(nq):
    m = int(rng.integers(10_000, 11_536))
    lists.append(np.unique(rng.integers(0, n, size=m + 400, dtype=np.uint32))[:m])
picks = rng.choice(n, 64, replace=False)
try:
    _lib.tuning_get("AH_RERANK_SCREEN_DIFF")
    settings = [("diff 0", dict(AH_RERANK_SCREEN_DIFF=0)), ("diff 1", dict(AH_RERANK_SCREEN_DIFF=1))] * 2
except Exception:
    settings = [("parent", {})] * 2

for cls in (distances.Euclidean, distances.Manhattan):
    for dist, dist_name in ((1, "uniform"), (4, "clustered")):
        ds = Dataset(cls, dims, n)
        ds.fill_synthetic(42, dist, n)
        ds.finalize()
        queries = np.tile(np.stack([ds.item_vector(int(i)) for i in picks]), (nq // 64 + 1, 1))[:nq]
        batches = []
        for b in range(0, nq, 125):
            off = np.zeros(126, dtype=np.uint64)
            off[1:] = np.cumsum([len(l) for l in lists[b:b + 125]])
            batches.append((queries[b:b + 125], (np.concatenate(lists[b:b + 125]), off)))
        ref = None
        for label, knobs in settings:
            with _lib.tuning(**knobs):
                ds.rerank_stats(reset=True)
                for q, l in batches:  # every shape of the timed window once (and, at 1, the binary16 copy of the rows)
                    ds.rerank_batch(q, l, k)
                ds.rerank_stats(reset=True)
                diff = ds.rerank_diff_stats(reset=True) if knobs else None
                times = []
                for rep in range(7):
                    t0 = time.perf_counter()
                    outs = [ds.rerank_batch(q, l, k) for q, l in batches]
                    times.append(time.perf_counter() - t0)
                st = ds.rerank_stats(reset=True)
                diff = ds.rerank_diff_stats(reset=True) if knobs else None
            got = np.concatenate([o[0] for o in outs]).tobytes() + np.concatenate([o[1] for o in outs]).tobytes()
            ref = ref or got
            el = sorted(times)[len(times) // 2]
            print(json.dumps({"metric": cls.__name__, "rows": dist_name, "setting": label, "queries_per_s": round(nq / el),
                              "ms_per_1000_queries_median_of_7": round(el * 1e3, 2), "identical_to_first": got == ref,
                              "survivors_per_screened_query": round(st["survivors"] / max(1, st["queries_screened"]), 1),
                              "queries_screened_per_pass": st["queries_screened"] // 7,
                              "sub_batches_overflowed": diff["chunks_overflowed"] if diff else 0,
                              "switched_off": diff["switched_off"] if diff else 0}), flush=True)
        ds.close()
