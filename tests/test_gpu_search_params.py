"""The batched search in which every query names its own count, search_k and oversampling besides its filter
(ah_search_batch_params), against the oracle's `nns_by_leaf` (src/reader.rs:317-401) and against ah_search_batch.

The contract: query q returns exactly what ah_search_batch returns for it alone with params[q] under the id list of its filter —
the same ids, distance bits and count — whatever else is in the call and however the call is cut.  Every query of every call
is compared with ah_search_batch called for it alone, and with the oracle where its effective search_k is at most 60 000 (plus
a fixed sample of ten of the larger ones).

The references are made once per world and shared.  They set the time of the 300-query case, the first to ask for all of them:
about a fifth of the queries draw a search_k that takes in the whole forest (720 000, 2^40), and ah_search_batch serves such a
query alone in 60 - 120 ms; the eight 300-query calls of the case itself take under a second each."""
import ctypes as C

import numpy as np
import pytest

from arroy_amd import Dataset, _lib, shard
from arroy_amd import distances as D
from oracle import oracle as O
from test_gpu_search_filters import DEVICE, OOM, U32_MAX, bits, filter_lists, same, sweep
from test_search_filters_cpu import NO_FILTER
from test_search_params_cpu import BATCH_TOPK_MAX, extent, plan, stats_of

pytestmark = pytest.mark.gpu

N, DIMS, TREES = 60_000, 200, 12  # reaches every descent tier and both dedup paths; desc_len = 720 000, leaves of <= 200 ids
NQ = 300
# 16 100 / 16 400: either side of the 16 384-entry buffer the LDS sort holds; 720 000 = desc_len; 2^40 is clamped to it
SK_LADDER = (0, 1, 199, 1500, 16_100, 16_400, 60_000, 720_000, 2**40)
# 1024 / 1025: the selection's capacity and one more; 2049 leaves the batched top-k
COUNT_LADDER = (1, 10, 25, 100, 1024, 1025, 2048, 2049, 5000)
OVER_LADDER = (0, 1, 4)
ORACLE_MAX_SK, ORACLE_SAMPLE = 60_000, 10

WORLDS = {"cosine": (D.Cosine, O.COSINE, False),                     # the screened leaf tiles
          "euclidean_sparse_ids": (D.Euclidean, O.EUCLIDEAN, True),  # ids up to u32::MAX: the sorted path
          "bq_cosine": (D.BinaryQuantizedCosine, O.BQ_COSINE, False)}  # default oversampling 3


def row_bytes(metric, dims):
    if metric is D.BinaryQuantizedCosine:
        return (((dims + 63) // 64 + 1) & ~1) * 8
    return ((dims + 31) & ~31) * 4


class World:
    def __init__(self, metric, ometric, sparse, n=N, dims=DIMS, trees=TREES, vecs=None, nq=NQ):
        vecs = O.synth(7, 2, n, dims) if vecs is None else vecs
        if sparse:  # ascending ids with gaps, the last one u32::MAX (src/tests/writer.rs:161-179)
            ids = (np.arange(n, dtype=np.uint64) * 3 + (np.arange(n, dtype=np.uint64) % 2)).astype(np.uint32)
            ids[-1] = U32_MAX
        else:
            ids = np.arange(n, dtype=np.uint32)
        self.metric, self.ids, self.vecs = metric, ids, vecs
        self.ds = Dataset(metric, dims, n)
        self.ds.upload_vectors(ids, vecs)
        self.od = O.Data(ometric, vecs, ids=ids if sparse else None)
        self.ds.finalize()
        self.forest = self.ds.build_forest(shard.tree_seeds(7, range(trees)))
        self.index = self.ds.create_index(self.forest)
        self.view = O.forest_view(self.forest)
        rng = np.random.default_rng(3)
        finite = np.flatnonzero(np.isfinite(vecs).all(axis=1))
        self.queries = (vecs[rng.choice(finite, nq, replace=False)] + rng.standard_normal((nq, dims)).astype(np.float32) * np.float32(0.1)).astype(np.float32)
        self.lists = filter_lists(ids)
        self.filters = [self.index.make_filter(x, sorted=True) for x in self.lists]
        self.slots = rng.integers(0, len(self.lists) + 1, nq).astype(np.uint32)
        self.slots[self.slots == len(self.lists)] = NO_FILTER
        self.slots[:8] = [0, NO_FILTER, 2, 1, 6, 3, 4, 5]  # the small calls see every kind too
        # per-query values from the ladders; the first 16 queries hold every rung once
        self.sks = rng.choice(np.array(SK_LADDER, dtype=np.int64), nq)
        self.counts = rng.choice(np.array(COUNT_LADDER, dtype=np.int64), nq)
        self.overs = rng.choice(np.array(OVER_LADDER, dtype=np.int64), nq)
        pin = min(16, nq)
        self.sks[:pin] = (list(SK_LADDER) + list(SK_LADDER[::-1][:7]))[:pin]
        self.counts[:pin] = (list(COUNT_LADDER[4:]) + list(COUNT_LADDER[:4]) + list(COUNT_LADDER[2:9]))[:pin]
        self.overs[:pin] = [0, 1, 4, 0, 0, 1, 4, 1, 0, 4, 1, 0, 4, 0, 1, 0][:pin]
        self.set_extents()
        self._truth, self._alone = {}, {}

    def set_extents(self):
        """The effective search_k and candidate-buffer stride of every query, as the host derives them."""
        info = self.index.export_info()
        nodes = self.index.export(normals=False)["nodes"]
        self.desc_len, self.max_desc = info["desc_len"], int(nodes["count"][nodes["kind"] == 1].max())
        ext = [extent(c, s, o, info["n_trees"], self.desc_len, self.max_desc, 3 if self.metric is D.BinaryQuantizedCosine else 1)
               for c, s, o in zip(self.counts, self.sks, self.overs)]
        self.sk_eff = np.array([e[0] for e in ext], dtype=np.int64)
        self.stride = np.array([e[1] for e in ext], dtype=np.int64)
        self.row_bytes = row_bytes(self.metric, self.vecs.shape[1])
        large = np.flatnonzero(self.sk_eff > ORACLE_MAX_SK)
        self.oracle_queries = set(np.flatnonzero(self.sk_eff <= ORACLE_MAX_SK).tolist()) | set(large[::max(1, large.size // ORACLE_SAMPLE)][:ORACLE_SAMPLE].tolist())

    def cand(self, qi):
        return None if self.slots[qi] == NO_FILTER else self.lists[int(self.slots[qi])]

    def truth(self, qi):
        """(ids, distance bits) of query qi with its own values under its filter's list, by the oracle."""
        if qi not in self._truth:
            qv, qh = self.od.query_leaf(self.queries[qi])
            want, _ = O.search(self.od, self.forest, qv, qh, int(self.counts[qi]), int(self.sks[qi]), int(self.overs[qi]), self.cand(qi),
                               candidates_sorted=True, want_candidates=False, view=self.view)
            self._truth[qi] = ([i for i, _ in want], np.array([d for _, d in want], dtype=np.float32).view(np.uint32).tolist())
        return self._truth[qi]

    def alone(self, qi):
        """ah_search_batch for query qi alone: (ids, distance bits, count), the row `count` wide and padded."""
        if qi not in self._alone:
            oi, od, oc = self.index.search(int(self.counts[qi]), queries=self.queries[qi:qi + 1], search_k=int(self.sks[qi]),
                                           oversampling=int(self.overs[qi]), raw=True, candidates=self.cand(qi), candidates_sorted=True)
            self._alone[qi] = (oi[0].copy(), bits(od[0]).copy(), int(oc[0]))
        return self._alone[qi]

    def check(self, got, sel, what):
        """Every query of the call `got` served the queries `sel` with: ah_search_batch alone, the oracle, the padding."""
        oi, od, oc = got
        assert oi.shape == od.shape and oi.shape[0] == len(sel) and oi.shape[1] >= int(self.counts[sel].max())
        for pos, qi in enumerate(sel):
            qi, c = int(qi), int(self.counts[qi])
            ai, ad, ac = self.alone(qi)
            about = (what, qi, c, int(self.sks[qi]), int(self.overs[qi]), int(self.slots[qi]))
            assert int(oc[pos]) == ac and ac <= c, about
            assert np.array_equal(oi[pos, :c], ai) and np.array_equal(bits(od[pos, :c]), ad), about
            assert (oi[pos, ac:] == U32_MAX).all() and (bits(od[pos, ac:]) == U32_MAX).all(), about
            if qi in self.oracle_queries:
                ids, dist = self.truth(qi)
                assert ac == len(ids) and ai[:ac].tolist() == ids and ad[:ac].tolist() == dist, ("oracle",) + about

    def call(self, nq, **tun):
        with _lib.tuning(**tun):
            for reset in (self.index.params_stats, self.index.stats, self.index.filter_stats):
                reset(reset=True)
            got = self.index.search_params(self.counts[:nq], queries=self.queries[:nq], search_ks=self.sks[:nq], oversamplings=self.overs[:nq],
                                           filters=self.filters, filter_of_query=self.slots[:nq], raw=True)
            return got, self.index.params_stats(), self.index.stats()

    def planned(self, nq, group_min, sort):
        batches = plan(self.stride[:nq], self.counts[:nq], self.slots[:nq], group_min, sort, self.row_bytes)
        return batches, stats_of(batches, self.counts[:nq], self.sk_eff[:nq])

    def close(self):
        self.index.close()  # (closes its filters first)
        self.forest.close()
        self.ds.close()


_worlds = {}


def get_world(name):
    if name not in _worlds:
        _worlds[name] = World(*WORLDS[name])
    return _worlds[name]


@pytest.fixture(scope="module", autouse=True)
def close_worlds():
    yield
    for w in _worlds.values():
        w.close()
    _worlds.clear()


@pytest.fixture(scope="module", params=list(WORLDS), ids=list(WORLDS))
def world(request):
    return get_world(request.param)


def test_every_rung_is_among_the_first_sixteen_queries_and_nothing_is_left_out(world):
    w = world
    assert set(w.sks[:16].tolist()) == set(SK_LADDER) and set(w.counts[:16].tolist()) == set(COUNT_LADDER)
    assert set(w.overs[:16].tolist()) == set(OVER_LADDER)
    assert set(w.sks.tolist()) == set(SK_LADDER) and set(w.counts.tolist()) == set(COUNT_LADDER)
    assert w.desc_len == N * TREES and w.max_desc <= DIMS
    assert len(w.oracle_queries) >= int((w.sk_eff <= ORACLE_MAX_SK).sum()) + min(ORACLE_SAMPLE, int((w.sk_eff > ORACLE_MAX_SK).sum()))


@pytest.mark.parametrize("nq", (1, 5, 64, NQ))
def test_varied_calls_equal_the_oracle_however_they_are_cut(world, nq):
    w = world
    sel = np.arange(nq)
    gmin = _lib.tuning_get("AH_SEARCH_FILTER_GROUP_MIN")[0]
    got, pst, _ = w.call(nq)
    w.check(got, sel, ("default", nq))
    batches, want = w.planned(nq, gmin, 1)
    assert pst == want, (nq, pst, want)
    if nq >= 16:
        assert pst["varied_batches"] >= 1 and pst["big_count_queries"] == int((w.counts[:nq] > BATCH_TOPK_MAX).sum())
    # the caller's order inside a run: the eight octets of one descent wave hold search_k 1 next to 720 000
    variants = [("caller's order", dict(AH_SEARCH_PARAMS_SORT=0), gmin, 0),
                ("all uniform", dict(AH_SEARCH_FILTER_GROUP_MIN=1), 1, 1),
                ("all mixed", dict(AH_SEARCH_FILTER_GROUP_MIN=nq + 1), nq + 1, 1),
                ("octet descent", dict(AH_SEARCH_WAVE=0), gmin, 1),
                ("no leaf tiles", dict(AH_SEARCH_TILES=0), gmin, 1),
                ("no screen", dict(AH_SEARCH_SCREEN=0), gmin, 1)]
    for name, tun, group_min, sort in variants:
        other, pst, sst = w.call(nq, **tun)
        same(other, got, (name, nq))
        assert pst == w.planned(nq, group_min, sort)[1], (name, nq, pst)
        if name == "octet descent":
            assert sst["descent_octet_lds"] + sst["descent_octet_global"] == nq, (nq, sst)
        if name == "no leaf tiles":
            assert sst["rerank_tiles"] == 0 and sst["rerank_sorted"] == nq, (nq, sst)
    w.ds.query_screen_verify(reset=True)
    ver, _, _ = w.call(nq, AH_SCREEN_VERIFY=1)
    same(ver, got, ("verify", nq))
    assert w.ds.query_screen_verify()["violations"] == 0


def tile_friendly(w, nq):
    """Counts <= 1024 and search_k <= 16 100, every one explicit; a count of 1024 — the selection's capacity — only with a
    search_k under which a query cannot have more candidates than that."""
    rng = np.random.default_rng(12)
    counts = rng.choice(np.array([1, 10, 25, 100], dtype=np.int64), nq)
    sks = rng.choice(np.array([1, 199, 1500, 16_100] if nq > 64 else [1, 199, 1500], dtype=np.int64), nq)
    at_capacity = np.arange(2, nq, 7)
    counts[at_capacity], sks[at_capacity] = 1024, np.where(np.arange(at_capacity.size) % 2 == 0, 199, 1)
    assert np.unique(counts).size > 1 and np.unique(sks).size > 1 and counts.max() == 1024
    return counts, sks


@pytest.mark.parametrize("nq", (NQ, 5))
def test_tiles_stay_open_to_varied_sub_batches(nq):
    w = get_world("cosine")
    counts, sks = tile_friendly(w, nq)
    for reset in (w.index.params_stats, w.index.stats):
        reset(reset=True)
    got = w.index.search_params(counts, queries=w.queries[:nq], search_ks=sks, raw=True)
    pst, sst = w.index.params_stats(), w.index.stats()
    assert pst["batches"] == 1 and pst["varied_batches"] == 1 and pst["varied_queries"] == nq, pst
    assert sst["rerank_tiles"] == nq and sst["rerank_sorted"] == 0 and sst["fallback_chunks"] == 0, sst
    if nq == 5:  # the small-submission path: a block (or several) per query, its own search_k in each
        assert sst["descent_block"] == 5 and sst["descent_octet_lds"] + sst["descent_octet_global"] == 0, sst
    for qi in range(nq):
        c = int(counts[qi])
        oi, od, oc = w.index.search(c, queries=w.queries[qi:qi + 1], search_k=int(sks[qi]), raw=True)
        assert int(got[2][qi]) == int(oc[0]) and np.array_equal(got[0][qi, :c], oi[0]) and np.array_equal(bits(got[1][qi, :c]), bits(od[0])), qi
        assert (got[0][qi, int(oc[0]):] == U32_MAX).all() and (bits(got[1][qi, int(oc[0]):]) == U32_MAX).all(), qi
        if qi % 10 == 0:
            qv, qh = w.od.query_leaf(w.queries[qi])
            want, _ = O.search(w.od, w.forest, qv, qh, c, int(sks[qi]), 0, None, want_candidates=False, view=w.view)
            assert got[0][qi, :len(want)].tolist() == [i for i, _ in want] and int(oc[0]) == len(want), qi
            assert bits(got[1][qi, :len(want)]).tolist() == np.array([d for _, d in want], dtype=np.float32).view(np.uint32).tolist(), qi


@pytest.mark.parametrize("nq", (1, 5, 64, NQ))
def test_equal_params_take_the_paths_of_the_filters_entry_point(world, nq):
    w = world
    for count, sk, over in ((25, 1500, 0), (2049, 0, 1)):
        res = []
        for entry in ("params", "filters"):
            for reset in (w.index.params_stats, w.index.stats, w.index.filter_stats):
                reset(reset=True)
            if entry == "params":
                got = w.index.search_params(count, queries=w.queries[:nq], search_ks=sk, oversamplings=over, filters=w.filters,
                                            filter_of_query=w.slots[:nq], raw=True)
            else:
                got = w.index.search(count, queries=w.queries[:nq], search_k=sk, oversampling=over, filters=w.filters,
                                     filter_of_query=w.slots[:nq], raw=True)
            res.append((got, w.index.stats(), w.index.filter_stats(), w.index.params_stats()))
        same(res[0][0], res[1][0], (nq, count))
        assert res[0][1] == res[1][1], (nq, count, res[0][1], res[1][1])  # ah_search_stats, field by field
        assert res[0][2] == res[1][2], (nq, count, res[0][2], res[1][2])  # ah_filter_stats
        assert res[0][3]["calls"] == 1 and res[0][3]["varied_batches"] == 0 and res[0][3]["queries"] == nq, res[0][3]
        assert res[0][3]["batches"] == res[0][2]["uniform_batches"] + res[0][2]["mixed_batches"]
        assert res[1][3] == dict.fromkeys(res[1][3], 0), "ah_params_stats counts the new entry point's calls only"


def test_by_item_queries_with_per_query_values_and_filters(world):
    w = world
    items = w.ids[[3, N - 1, 1234, 777, 31_000, 9]]
    slots = np.array([1, 0, NO_FILTER, 0, 4, 2], dtype=np.uint32)
    counts, sks, overs = [25, 1, 2049, 1024, 100, 10], [1500, 0, 199, 16_400, 2**40, 0], [0, 4, 1, 0, 0, 1]
    got = w.index.search_params(counts, items=items, search_ks=sks, oversamplings=overs, filters=w.filters, filter_of_query=slots, raw=True)
    assert got[0].shape == (6, 2049)
    for qi in range(len(items)):
        cand = None if slots[qi] == NO_FILTER else w.lists[int(slots[qi])]
        oi, od, oc = w.index.search(counts[qi], items=items[qi:qi + 1], search_k=sks[qi], oversampling=overs[qi], raw=True,
                                    candidates=cand, candidates_sorted=True)
        c = counts[qi]
        assert int(got[2][qi]) == int(oc[0]) and np.array_equal(got[0][qi, :c], oi[0]) and np.array_equal(bits(got[1][qi, :c]), bits(od[0])), qi
        assert (got[0][qi, int(oc[0]):] == U32_MAX).all() and (bits(got[1][qi, int(oc[0]):]) == U32_MAX).all(), qi
    # the list form, and an item that is not stored
    as_lists = w.index.search_params(counts, items=items, search_ks=sks, oversamplings=overs, filters=w.filters, filter_of_query=slots)
    assert [len(r) for r in as_lists] == got[2].tolist() and [r[0][0] for r in as_lists if r] == [int(got[0][q, 0]) for q in range(6) if got[2][q]]
    if w.ids[-1] != U32_MAX:
        with pytest.raises(_lib.ArroyHipError, match="does not exist"):
            w.index.search_params(5, items=[int(w.ids[-1]) + 1])


def test_non_finite_distances_follow_the_positional_rule_per_query():
    """`median_based_top_k(v, k)` drops what is >= (f32::MAX, u32::MAX) after its first 2k items, so the result under a small k
    is no prefix of the result under a larger one: every query's own count reaches the sorted re-rank."""
    n, dims, trees = 3000, 32, 8
    rng = np.random.default_rng(9)
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    bad = rng.choice(n, 20, replace=False)
    for i, r in enumerate(bad):
        vecs[r, rng.choice(dims, 1 + i % 3, replace=False)] = np.float32(np.inf) if i % 2 == 0 else np.float32(np.nan)
    w = World(D.Euclidean, O.EUCLIDEAN, False, n=n, dims=dims, trees=trees, vecs=vecs, nq=12)
    try:
        w.slots[:] = NO_FILTER
        w.counts[:] = [1, 5, 40, 40, 1, 5, 5, 40, 1, 40, 5, 1]
        w.sks[:] = [100, 24_000, 100, 24_000, 24_000, 100, 24_000, 100, 100, 24_000, 24_000, 24_000]
        w.overs[:] = 0
        w.set_extents()
        assert len(w.oracle_queries) == 12
        got, pst, sst = w.call(12)
        w.check(got, np.arange(12), "non-finite")
        assert pst["batches"] == 1 and pst["varied_batches"] == 1, pst
        assert sst["fallback_non_finite"] >= 1 and sst["rerank_sorted"] == 12, sst
        for tun in (dict(AH_SEARCH_TILES=0), dict(AH_SEARCH_PARAMS_SORT=0), dict(AH_SEARCH_WAVE=0)):
            same(w.call(12, **tun)[0], got, tun)
    finally:
        w.close()


def test_the_callers_order_with_rows_narrower_than_out_stride():
    """A call whose sub-batches keep the caller's order but stage rows narrower than out_stride: the queries are read where the
    caller put them and the results are copied back row by row.  Unfiltered queries, batched counts before big ones, strides
    ascending inside each kind: two sub-batches, [0, 1] of rows 25 wide and [2, 3] of rows 3000 wide, in an output 3000 wide;
    then the same four queries with the order switch off and an out_stride beyond the largest count, through the C ABI."""
    w = World(D.Euclidean, O.EUCLIDEAN, False, n=400, dims=32, trees=5, nq=8)  # (the calls take its first four queries)
    try:
        w.slots[:] = NO_FILTER
        w.counts[:] = [10, 25, 2049, 3000] * 2
        w.sks[:] = [100, 400, 100, 400] * 2
        w.overs[:] = 0
        w.set_extents()
        assert len(w.oracle_queries) == 8
        for sort in (1, 0):
            batches, want = w.planned(4, _lib.tuning_get("AH_SEARCH_FILTER_GROUP_MIN")[0], sort)
            assert [b.tolist() for _k, b in batches] == [[0, 1], [2, 3]]  # the caller's order, and a sub-batch of rows 25 wide
            got, pst, sst = w.call(4, AH_SEARCH_PARAMS_SORT=sort)
            assert got[0].shape == (4, 3000)
            w.check(got, np.arange(4), ("caller's order, narrow rows", sort))
            assert pst == want and pst["batches"] == 2 and pst["varied_queries"] == 4 and pst["big_count_queries"] == 2, pst
            assert sst["chunks"] == 2 and sst["queries"] == 4, sst
        L = _lib.lib()
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        params = (_lib.AhQueryParams * 4)()
        for i in range(4):
            params[i].search_k, params[i].count, params[i].oversampling = int(w.sks[i]), int(w.counts[i]), 0
        q = np.ascontiguousarray(w.queries[:4])
        stride = 3000 + 11
        oi, od, oc = np.zeros((4, stride), np.uint32), np.zeros((4, stride), np.float32), np.full(4, 77, np.uint32)
        with _lib.tuning(AH_SEARCH_PARAMS_SORT=0):
            _lib.check(L.ah_search_batch_params(w.index._h, p(q), None, 4, params, stride, C.POINTER(C.c_void_p)(), 0, None, p(oi), p(od), p(oc)))
        w.check((oi, od, oc), np.arange(4), "caller's order, out_stride beyond every count")
        same((oi[:, :3000], od[:, :3000], oc), got, "the wider rows hold the same results")
    finally:
        w.close()


def test_a_varied_call_survives_every_allocation_failure():
    """Injected allocation failures return a status by design (they are not device faults): every allocation of one varied
    ah_search_batch_params call fails once, the next call gives the right bits and no HBM is leaked."""
    ref = get_world("cosine")
    w = World(*WORLDS["cosine"])  # (a warmed-up context allocates nothing on the device: a dataset, and contexts, of its own)
    try:
        # uniform and mixed sub-batches, varied ones, big counts; buffers of a few thousand candidates
        sel = np.flatnonzero(w.sk_eff <= 16_400)
        assert sel.size >= 60 and (w.counts[sel] > BATCH_TOPK_MAX).any() and np.unique(w.slots[sel]).size == len(w.lists) + 1

        def op():
            return w.index.search_params(w.counts[sel], queries=w.queries[sel], search_ks=w.sks[sel], oversamplings=w.overs[sel],
                                         filters=w.filters, filter_of_query=w.slots[sel], raw=True)
        seen = sweep(op)
        assert len(seen) >= 4 and all(s in (OOM, DEVICE) for s in seen), seen  # host vectors at the least
        assert OOM in seen
        got = op()
        ref.check(got, sel, "after the sweeps")  # (the same data and seeds: the module's world holds the references)
        assert w.index.params_stats()["varied_batches"] >= 1
    finally:
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        w.close()


def test_short_and_long_rows():
    w = get_world("cosine")
    L = _lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    sel = np.array([0, 1, 2, 3, 16, 17, 18])
    nq, stride = sel.size, int(w.counts[sel].max()) + 37
    params = (_lib.AhQueryParams * nq)()
    for i, qi in enumerate(sel):
        params[i].search_k, params[i].count, params[i].oversampling = int(w.sks[qi]), int(w.counts[qi]), int(w.overs[qi])
    q = np.ascontiguousarray(w.queries[sel])
    slots = np.ascontiguousarray(w.slots[sel])
    handles = (C.c_void_p * len(w.filters))(*[f._handle() for f in w.filters])
    oi, od, oc = np.zeros((nq, stride), np.uint32), np.zeros((nq, stride), np.float32), np.full(nq, 77, np.uint32)
    _lib.check(L.ah_search_batch_params(w.index._h, p(q), None, nq, params, stride, handles, len(w.filters), p(slots), p(oi), p(od), p(oc)))
    w.check((oi, od, oc), sel, "out_stride beyond the largest count")
    assert (oi[:, int(w.counts[sel].max()):] == U32_MAX).all()
    # count = 5000 under search_k = 1: one leaf of every tree at the most, a short row
    oi, od, oc = w.index.search_params([5000, 10], queries=w.queries[:2], search_ks=[1, 1500], raw=True)
    assert oi.shape == (2, 5000) and 0 < oc[0] <= w.max_desc and oc[1] == 10
    one = w.index.search(5000, queries=w.queries[:1], search_k=1, raw=True)
    assert int(one[2][0]) == int(oc[0]) and np.array_equal(one[0][0], oi[0]) and np.array_equal(bits(one[1][0]), bits(od[0]))
    assert (oi[1, 10:] == U32_MAX).all() and np.isnan(od[1, 10:]).all()
    # nq == 0 is AH_OK and asks nothing of params
    assert L.ah_search_batch_params(w.index._h, p(q), None, 0, None, 0, handles, 0, None, p(oi), p(od), p(oc)) == 0
