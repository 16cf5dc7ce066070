"""What one sub-batch of a search chooses and launches (plan_chunk in arroy_amd/csrc/search_plan.h and the stages of
search_chunk in search.hip), pinned to what the search did before the plan was written down as one function.

Small indexes (20 000 rows, one per metric, built once per module) and one search call per case at the edges of the plan:
the query counts where the small tiles, k_descend_multi, the block descent / k_units_small and the int8 screen begin or end,
8 / 9 / 3 trees, 31 / 32 dimensions, rows of more than 32 KiB, the counts around kSelectCap and the tournament top-k, uniform filters on either side
of the 0.35 and 0.05 shares, a mixed, a varied and a transient-filter call, every metric family, ids past the LDS bitmap, and
every kernel-selecting knob flipped once on the one-query and the eight-query Cosine call.  After each call the whole
ah_search_stats (read with reset) and a hash of ids, distance bits and counts equal tests/golden/search_plan_stats.json,
recorded with these same calls on commit 403e52f (the parent of the change that introduced the plan).  They are exact counts
and hashes: no tolerance.

One counter is not a function of the call where the int8 stage of the screen runs (`rerank_screened8` != 0), and is held to
less there and only there: `screen_survivors`.  k_flag_duplicates keeps whichever occurrence of an id sets its bit first (an
atomicOr race between the waves of a block); with two stages the occurrences of an id can carry the bound of the int8 tiles or
of the binary16 tiles, whichever its leaf took, so a few candidates near the threshold survive or not from run to run — results
unchanged.  Three recordings of commit 403e52f differed from one another in it and in nothing else, in five of the twelve cases
that ran the int8 stage (by up to 8 of 42 885) and in none of the others; in those twelve it has to be zero exactly where the
recording's is, in every other case it is exact like the rest."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

from arroy_amd import _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from oracle import oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "search_plan_stats.json")
N = 20_000
NO_FILTER = 0xFFFFFFFF
KNOBS = [{"AH_SEARCH_TILES": 0}, {"AH_SEARCH_SCREEN": 0}, {"AH_SEARCH_SCREEN8": 1, "AH_SEARCH_SCREEN8_MIN_QUERIES": 2},
         {"AH_SEARCH_BITMAP": 0}, {"AH_SEARCH_WAVE": 0}, {"AH_SEARCH_MULTI": 0}, {"AH_SEARCH_MULTI_OWN_UNITS": 0},
         {"AH_SEARCH_SINGLE_FUSED": 0}, {"AH_SEARCH_FUSED_FLAG": 0}, {"AH_SEARCH_FUSED_PREPARE": 0}, {"AH_SEARCH_FLAT_TILES": 0},
         {"AH_SEARCH_ITEM_LIST": 0}, {"AH_SEARCH_SMALL_GATE": 0}, {"AH_SEARCH_SPIN_WAIT": 0}, {"AH_SEARCH_STATUS_WIPE": 0}]


class World:
    """One dataset, its forests by number of trees, and queries near its rows."""

    def __init__(self, cls, dims, n=N, sparse_ids=False):
        from arroy_amd import Dataset
        self.dims, self.n = dims, n
        self.ds = Dataset(cls, dims, n)
        if sparse_ids:  # explicit ids, the largest past the 1 277 952 the LDS bitmap holds
            self.ids = (np.arange(n, dtype=np.uint64) * 70 + 3).astype(np.uint32)
            self.ds.upload_vectors(self.ids, O.synth(dims, 1, n, dims))
        else:
            self.ids = np.arange(n, dtype=np.uint32)
            self.ds.fill_synthetic(dims, 1, n)
        if cls is D.DotProduct:
            self.ds.preprocess_dot()
        self.ds.finalize()
        self.indexes = {}

    def index(self, trees):
        if trees not in self.indexes:
            forest = self.ds.build_forest(list(range(900, 900 + trees)))
            self.indexes[trees] = (self.ds.create_index(forest), forest)
        return self.indexes[trees][0]

    def queries(self, nq):
        rows = O.synth(self.dims, 1, nq, self.dims, first_item=37)
        return (rows + np.float32(0.05) * O.synth(5, 1, nq, self.dims)).astype(np.float32)

    def share(self, share):
        """An ascending id list that holds `share` of the stored ids."""
        rng = np.random.default_rng(int(share * 1000))
        return np.sort(rng.choice(self.ids, int(round(share * self.n)), replace=False)).astype(np.uint32)

    def close(self):
        for index, forest in self.indexes.values():
            index.close()
            forest.close()
        self.ds.close()


def outcome(index, res):
    ids, dist, counts = res
    h = hashlib.sha256()
    for a in (ids, dist, counts):
        h.update(np.ascontiguousarray(a).tobytes())
    return {"stats": {f: v for f, v in index.stats(reset=True).items() if v}, "hash": h.hexdigest()}  # (the golden file leaves zeros out)


def run(world, trees, nq, count=10, search_k=400, knobs=None, **kw):
    index = world.index(trees)
    index.stats(reset=True)
    with _lib.tuning(**(knobs or {})):
        return outcome(index, index.search(count, queries=world.queries(nq), search_k=search_k, raw=True, **kw))


def collect_cosine():
    w = World(D.Cosine, 64)
    got = {}
    for nq in (1, 2, 8, 9, 32, 33, 64, 65, 4097):  # (4097: one sub-batch past the most queries of one)
        got[f"nq{nq}"] = run(w, 9, nq)
    for nq in (1, 8):
        got[f"trees8/nq{nq}"] = run(w, 8, nq)  # one block of k_descend_multi: the block descent
        got[f"trees3/nq{nq}"] = run(w, 3, nq, search_k=3000)  # the small gate refuses the block descent
    for nq in (2, 8):  # candidate buffers long enough for every query's descent to write its own units
        got[f"own_units/nq{nq}"] = run(w, 9, nq, search_k=1500)
    for count, sk in ((1024, 2000), (1025, 900), (1025, 3000), (2048, 5000), (2049, 5000)):
        got[f"count{count}/sk{sk}"] = run(w, 9, 3, count=count, search_k=sk)
    index = w.index(9)
    filters = {s: index.make_filter(w.share(s), sorted=True) for s in (0.5, 0.36, 0.34, 0.06, 0.04, 0.03)}
    for s, f in filters.items():
        for nq in (1, 8, 70):
            got[f"share{s}/nq{nq}"] = run(w, 9, nq, candidates=f)
    fl = [filters[0.5], filters[0.34], filters[0.06]]
    got["mixed"] = run(w, 9, 12, filters=fl, filter_of_query=[0, 1, 2, NO_FILTER] * 3)
    index.stats(reset=True)
    got["varied"] = outcome(index, index.search_params([10, 3, 40, 10, 1, 25] * 2, queries=w.queries(12),
                                                       search_ks=[400, 100, 900, 0, 50, 400] * 2, raw=True))
    for nq in (15, 16):  # the transient filter of ah_search_batch
        got[f"transient/nq{nq}"] = run(w, 9, nq, candidates=w.share(0.5), candidates_sorted=True)
    index.stats(reset=True)
    got["by_item"] = outcome(index, index.search(10, items=[5, 77, 19_999, 400, 5], search_k=400, raw=True))
    for f in filters.values():
        f.close()
    for knobs in KNOBS:
        for nq in (1, 8):
            got["/".join(f"{k}={v}" for k, v in knobs.items()) + f"/nq{nq}"] = run(w, 9, nq, knobs=knobs)
    w.close()
    return got


def collect_metrics():
    got = {}
    for name, cls, dims in (("dot64", D.DotProduct, 64), ("euclidean32", D.Euclidean, 32), ("euclidean31", D.Euclidean, 31),
                            ("cosine32", D.Cosine, 32), ("cosine31", D.Cosine, 31), ("manhattan64", D.Manhattan, 64),
                            ("bq_cosine64", D.BinaryQuantizedCosine, 64)):
        w = World(cls, dims)
        for nq in (1, 8, 70):
            got[f"{name}/nq{nq}"] = run(w, 9, nq)
        w.close()
    return got


def collect_ids():
    """Ids past the LDS bitmap: the hash flagger; a stride past what that holds: neither, the sorted path."""
    w = World(D.Cosine, 64, sparse_ids=True)
    got = {}
    for nq in (1, 8, 70):
        got[f"hash/nq{nq}"] = run(w, 9, nq)
    got["neither/nq2"] = run(w, 9, 2, search_k=30_000)
    w.close()
    return got


def collect_wide():
    """A row of more than 32 KiB: no wave descent, and the query leaf of the screened selection (its dynamic LDS) is past what a
    launch may ask for without the opt-in — fused into the selection for one query, unfused past k_units_small's 64 queries."""
    w = World(D.Cosine, 8200, n=3000)
    got = {f"nq{nq}": run(w, 9, nq) for nq in (1, 70)}
    w.close()
    return got


COLLECT = {"cosine": collect_cosine, "metrics": collect_metrics, "ids": collect_ids, "wide": collect_wide}


@pytest.mark.parametrize("group", sorted(COLLECT))
def test_every_sub_batch_chooses_and_answers_what_it_did(group):
    with open(GOLDEN) as f:
        want = json.load(f)[group]
    got = COLLECT[group]()
    assert sorted(got) == sorted(want), group
    for key in want:
        if want[key]["stats"].get("rerank_screened8"):  # (the int8 stage ran: see above)
            survivors = got[key]["stats"].pop("screen_survivors", 0), want[key]["stats"].pop("screen_survivors", 0)
            assert (survivors[0] == 0) == (survivors[1] == 0), f"{group} {key}: screen_survivors {survivors[0]}, recorded {survivors[1]}"
        assert got[key] == want[key], f"{group} {key}: {got[key]} != {want[key]}"
