"""Mixed sub-batches through the leaf tiles (AH_SEARCH_MIXED_TILES=1; DESIGN.md §4 "Mixed sub-batches through the leaf tiles"):
every query of a call whose queries are under different filters returns the oracle's ids and distance BITS for its own filter's
list, the statistics say k_leaf_tiles_mixed answered, and the switch at 0 gives the same bits from the sorted path.

6000 rows under 6 trees, leaves of up to `dims` ids: two slabs of 64 positions at 72 dimensions (the rank base across a slab
boundary), four at 200.  300 queries, 15 small perturbations of each of 20 rows, so that many queries meet in the same leaves;
the filters are dealt round robin, so the queries of one row are under different ones."""
import functools

import numpy as np
import pytest

from arroy_amd import Dataset, _lib, shard
from arroy_amd import distances as D
from oracle import oracle as O
from test_gpu_search_filters import bits, same
from test_search_filters_cpu import NO_FILTER

pytestmark = pytest.mark.gpu
N, TREES, COUNT, SK, NQ = 6000, 6, 10, 600, 300
U32_MAX = 0xFFFFFFFF
EVEN, ODD, LOWER, EVERY20, EVERY500, ALL, EMPTY, BEYOND = range(8)
# The slots a call deals round robin.  "all": every filter, the every-500th first, so that the calls of two queries hold it too
# — it keeps under 5 % of the ids (and the empty list none), so the whole sub-batch takes the octet descent.  "wave": without
# those two, every share at 5 % or more: the wave descents.  "halves": shares of a half or more, where the plan's estimate of
# the leaves a query opens admits the block descent, k_units_small and the selection that flags duplicates itself.
DEALS = {"all": [EVERY500, EVEN, ODD, LOWER, EVERY20, ALL, EMPTY, BEYOND, NO_FILTER],
         "wave": [EVERY20, EVEN, ODD, LOWER, ALL, BEYOND, NO_FILTER],
         "halves": [EVEN, ODD, LOWER, NO_FILTER, ALL]}
# name: (metric, oracle's metric, dimensions, AH_SEARCH_SCREEN_DIFF, the last id of sparse ids or None)
TILED = {"cosine-200": (D.Cosine, O.COSINE, 200, 0, None),
         "dot-72": (D.DotProduct, O.DOT_PRODUCT, 72, 0, None),  # a binary16 pitch that is no whole number of kMidSteps steps
         "euclidean-72": (D.Euclidean, O.EUCLIDEAN, 72, 0, None),  # the f32 tile with a scalar tail (72 mod 32 = 8)
         "euclidean-200-diff": (D.Euclidean, O.EUCLIDEAN, 200, 1, None),
         "manhattan-72-diff": (D.Manhattan, O.MANHATTAN, 72, 1, None),
         # the hash dedup, the id -> row table and the edge of len_bits.  (The last id is u32::MAX - 1, not u32::MAX: with id
         # u32::MAX stored no sub-batch, uniform or mixed, is planned onto the tiles at all — the value is the duplicate mark of
         # both flaggers, ChunkPlan::hash_fits — so that world is below, among the plans that stay on the sorted path.)
         "euclidean-72-sparse": (D.Euclidean, O.EUCLIDEAN, 72, 0, U32_MAX - 1)}
SORTED = {"manhattan-72": (D.Manhattan, O.MANHATTAN, 72, 0, None),
          "bq-cosine-72": (D.BinaryQuantizedCosine, O.BQ_COSINE, 72, 0, None),
          "euclidean-72-sparse-max": (D.Euclidean, O.EUCLIDEAN, 72, 0, U32_MAX)}


class World:
    def __init__(self, metric, ometric, dims, diff, last_id):
        vecs = O.synth(7, 2, N, dims)
        ids = np.arange(N, dtype=np.uint32)
        if last_id is not None:  # ascending ids with gaps (src/tests/writer.rs:161-179)
            ids = (np.arange(N, dtype=np.uint64) * 3 + (np.arange(N, dtype=np.uint64) % 2)).astype(np.uint32)
            ids[-1] = last_id
        self.ds, self.od, self.diff = Dataset(metric, dims, N), O.Data(ometric, vecs, ids=None if last_id is None else ids), diff
        self.ds.upload_vectors(ids, vecs)
        if metric is D.DotProduct:
            self.ds.preprocess_dot()
            self.od.preprocess_dot()
        self.ds.finalize()
        self.forest = self.ds.build_forest(shard.tree_seeds(7, range(TREES)))
        with _lib.tuning(AH_SEARCH_SCREEN_DIFF=diff):
            self.index = self.ds.create_index(self.forest)
        self.view = O.forest_view(self.forest)
        rng = np.random.default_rng(3)
        anchors = vecs[rng.choice(N, NQ // 15, replace=False)]
        self.queries = (np.repeat(anchors, 15, axis=0) + rng.standard_normal((NQ, dims)).astype(np.float32) * np.float32(0.02)).astype(np.float32)
        if last_id is None:
            beyond = np.concatenate([ids[1::3], np.arange(N, N + 60, 3, dtype=np.uint32)])
        else:  # ... laced with ids that are not stored
            beyond = np.union1d(ids[1::3], np.setdiff1d(np.arange(0, 3000, dtype=np.uint32), ids)[::2]).astype(np.uint32)
        self.lists = [ids[::2].copy(), ids[1::2].copy(), ids[:N // 2].copy(), ids[::20].copy(), ids[::500].copy(), ids.copy(),
                      np.zeros(0, np.uint32), beyond]
        self.filters = [self.index.make_filter(x, sorted=True) for x in self.lists]
        self._truth = {}

    def truth(self, qi, slot, count=COUNT, sk=SK):
        """(ids, distance bits) of query qi under the list of `slot`, by the oracle."""
        key = (qi, slot, count, sk)
        if key not in self._truth:
            want, _ = O.search(self.od, self.forest, *self.od.query_leaf(self.queries[qi]), count, sk, 0, None if slot == NO_FILTER else self.lists[slot],
                               candidates_sorted=True, want_candidates=False, view=self.view)
            self._truth[key] = ([i for i, _ in want], bits(np.array([d for _, d in want], dtype=np.float32)).tolist())
        return self._truth[key]

    def is_oracles(self, got, slots, what, counts=None, sks=None):
        oi, od, oc = got
        for qi, slot in enumerate(slots):
            ids, dist = self.truth(qi, int(slot), *(() if counts is None else (int(counts[qi]), int(sks[qi]))))
            assert int(oc[qi]) == len(ids), (what, qi, int(slot), int(oc[qi]), len(ids))
            assert oi[qi, :len(ids)].tolist() == ids and bits(od[qi, :len(ids)]).tolist() == dist, (what, qi, int(slot))

    def call(self, slots, on, **tun):
        """One call that is ONE mixed sub-batch: (results, ah_search_stats, ah_filter_stats)."""
        nq = len(slots)
        with _lib.tuning(AH_SEARCH_MIXED_TILES=on, AH_SEARCH_SCREEN_DIFF=self.diff, AH_SEARCH_FILTER_GROUP_MIN=nq + 1, **tun):
            self.index.stats(reset=True), self.index.filter_stats(reset=True)
            got = self.index.search(COUNT, queries=self.queries[:nq], search_k=SK, raw=True, filters=self.filters, filter_of_query=slots)
            return got, self.index.stats(), self.index.filter_stats()


@functools.lru_cache(maxsize=None)
def world(name):
    return World(*{**TILED, **SORTED}[name])


def deal(name, nq):
    return np.resize(np.array(DEALS[name], dtype=np.uint32), nq)


@pytest.mark.parametrize("nq", [2, 5, 40, NQ])
@pytest.mark.parametrize("dealt", list(DEALS))
@pytest.mark.parametrize("name", list(TILED))
def test_mixed_calls_through_the_tiles_are_the_oracles(name, dealt, nq):
    w, slots = world(name), deal(dealt, nq)
    got, st, fst = w.call(slots, 1)
    print(name, dealt, nq, st)
    w.is_oracles(got, slots, (name, dealt, nq))
    assert fst["mixed_batches"] == 1 and fst["mixed_queries"] == nq and fst["uniform_batches"] == 0, fst
    assert st["rerank_tiles"] == nq and st["rerank_sorted"] == 0 and st["tile_visits"] > 0 and st["fallback_chunks"] == 0, st
    octet, nq_waves = st["descent_octet_lds"] + st["descent_octet_global"], st["descent_block"] + st["descent_wave_small"] + st["descent_wave_big"]
    assert (octet == nq and nq_waves == 0) if dealt == "all" else nq_waves > 0, st
    assert dealt != "halves" or nq > 40 or st["descent_block"] > 0, st
    if nq == NQ:  # every Q shape of the kernel: units of up to 4 visits (registers), of 5 - 8 and of 9 - 16 (operands through LDS)
        assert st["tile_units_16"] > 0 and st["tile_units_8"] > 0 and st["tile_units_4"] > 0, st
    off, st0, fst0 = w.call(slots, 0)
    same(got, off, "switch on vs off")
    assert st0["rerank_tiles"] == 0 and st0["rerank_sorted"] == nq and fst0["mixed_batches"] == 1, (st0, fst0)


@pytest.mark.parametrize("name,tun", [(n, {}) for n in SORTED] + [("cosine-200", {"AH_SEARCH_SCREEN": 0})])
def test_plans_that_stay_on_the_sorted_path_under_the_switch(name, tun, nq=40):
    w, slots = world(name), deal("all", nq)
    got, st, fst = w.call(slots, 1, **tun)
    w.is_oracles(got, slots, name)
    assert st["rerank_tiles"] == 0 and st["rerank_sorted"] == nq and fst["mixed_batches"] == 1 and fst["mixed_queries"] == nq, (st, fst)


def test_per_query_parameters_in_a_mixed_tile_call(name="dot-72", nq=40):
    w, slots = world(name), deal("wave", nq)
    counts, sks = np.resize([1, 10, 40], nq), np.resize([SK, SK // 2], nq)
    with _lib.tuning(AH_SEARCH_MIXED_TILES=1, AH_SEARCH_FILTER_GROUP_MIN=nq + 1):
        w.index.stats(reset=True)
        got = w.index.search_params(counts, queries=w.queries[:nq], search_ks=sks, filters=w.filters, filter_of_query=slots, raw=True)
        st = w.index.stats()
    w.is_oracles(got, slots, "varied", counts, sks)
    assert st["rerank_tiles"] == nq and st["fallback_chunks"] == 0, st


def test_the_screen_holds_its_bounds_in_a_mixed_tile_call(name="cosine-200", nq=40):
    w, slots = world(name), deal("wave", nq)
    got = w.call(slots, 1)[0]
    w.ds.query_screen_verify(reset=True)
    ver, st, _ = w.call(slots, 1, AH_SCREEN_VERIFY=1)
    assert st["rerank_tiles"] == nq and w.ds.query_screen_verify()["violations"] == 0, (st, w.ds.query_screen_verify())
    same(ver, got, "verified vs not")
