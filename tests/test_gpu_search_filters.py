"""Resident candidate filters (ah_filter_*) and the batched search in which every query names its own
(ah_search_batch_filters), against the oracle's `nns_by_leaf` under `candidates` (src/reader.rs:110-123, 341-374).

The contract: query q returns exactly what ah_search_batch returns for it alone under the id list of its filter — the same ids
and distance bits — whatever else is in the call and however the call is cut into uniform and mixed sub-batches.  Every query
of every call is compared (with the oracle, except in the large case, where the oracle takes a sample of 40 and per-filter
ah_search_batch calls cover all)."""
import threading

import numpy as np
import pytest

from arroy_amd import Dataset, Index, _lib, shard
from arroy_amd import distances as D
from oracle import oracle as O
from test_search_filters_cpu import NO_FILTER, plan

pytestmark = pytest.mark.gpu

N, DIMS, TREES = 60_000, 200, 12  # the shapes of test_gpu_small_calls.py's world
COUNT, SK = 25, 1500
OK, DEVICE, OOM = 0, 3, 4
U32_MAX = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what=""):
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y)), what


def filter_lists(ids):
    """The id lists of the suite's filters over the ascending stored ids `ids`: stored shares 0.5, 0.05 and 0.002 (below the
    wave descent's 5 % rule), an empty list, every id, a list whose tail lies beyond the largest stored id (or, where that id is
    u32::MAX, one laced with ids that are not stored), and a list of ids none of which is stored."""
    ids = np.asarray(ids, dtype=np.uint32)
    top = int(ids[-1])
    if top < U32_MAX - 100:
        beyond = np.concatenate([ids[1::3], np.arange(top + 1, top + 60, 3, dtype=np.uint32)])
        absent = np.arange(top + 2, top + 90, 2, dtype=np.uint32)
    else:  # sparse ids up to u32::MAX: the gaps between the stored ids
        gaps = np.setdiff1d(np.arange(0, 3000, dtype=np.uint32), ids)
        beyond = np.union1d(ids[1::3], gaps[::2]).astype(np.uint32)
        absent = gaps[1::2].astype(np.uint32)
    return [ids[::2].copy(), ids[::20].copy(), ids[::500].copy(), np.zeros(0, np.uint32), ids.copy(), beyond, absent]


WORLDS = [("cosine", D.Cosine, O.COSINE, False), ("dot", D.DotProduct, O.DOT_PRODUCT, False),
          ("euclidean", D.Euclidean, O.EUCLIDEAN, False), ("manhattan", D.Manhattan, O.MANHATTAN, False),
          ("bq_cosine", D.BinaryQuantizedCosine, O.BQ_COSINE, False), ("euclidean_sparse_ids", D.Euclidean, O.EUCLIDEAN, True)]


class World:
    def __init__(self, metric, ometric, sparse):
        vecs = O.synth(7, 2, N, DIMS)
        if sparse:  # ascending ids with gaps, the last one u32::MAX (src/tests/writer.rs:161-179)
            ids = (np.arange(N, dtype=np.uint64) * 3 + (np.arange(N, dtype=np.uint64) % 2)).astype(np.uint32)
            ids[-1] = U32_MAX
        else:
            ids = np.arange(N, dtype=np.uint32)
        self.ids, self.vecs = ids, vecs
        self.ds = Dataset(metric, DIMS, N)
        self.ds.upload_vectors(ids, vecs)
        self.od = O.Data(ometric, vecs, ids=ids if sparse else None)
        if metric is D.DotProduct:
            self.ds.preprocess_dot()
            self.od.preprocess_dot()
        self.ds.finalize()
        self.forest = self.ds.build_forest(shard.tree_seeds(7, range(TREES)))
        self.index = self.ds.create_index(self.forest)
        self.view = O.forest_view(self.forest)
        rng = np.random.default_rng(3)
        nq = 700
        self.queries = (vecs[rng.choice(N, nq, replace=False)] + rng.standard_normal((nq, DIMS)).astype(np.float32) * np.float32(0.1)).astype(np.float32)
        self.lists = filter_lists(ids)
        self.filters = [self.index.make_filter(x, sorted=True) for x in self.lists]
        self.slots = rng.integers(0, len(self.lists) + 1, nq).astype(np.uint32)
        self.slots[self.slots == len(self.lists)] = NO_FILTER
        self.slots[:8] = [0, NO_FILTER, 2, 1, 6, 3, 4, 5]  # the small calls see every kind too
        self._truth = {}

    def truth(self, qi):
        """(ids, distance bits) of query qi under its filter's list, by the oracle."""
        if qi not in self._truth:
            slot = int(self.slots[qi])
            qv, qh = self.od.query_leaf(self.queries[qi])
            want, _ = O.search(self.od, self.forest, qv, qh, COUNT, SK, 0, None if slot == NO_FILTER else self.lists[slot],
                               candidates_sorted=True, want_candidates=False, view=self.view)
            self._truth[qi] = ([i for i, _ in want], np.array([d for _, d in want], dtype=np.float32).view(np.uint32).tolist())
        return self._truth[qi]

    def check(self, got, nq, what):
        oi, od, oc = got
        for qi in range(nq):
            ids, dist = self.truth(qi)
            assert int(oc[qi]) == len(ids), (what, qi, int(self.slots[qi]), int(oc[qi]), len(ids))
            assert oi[qi, :len(ids)].tolist() == ids, (what, qi, int(self.slots[qi]))
            assert bits(od[qi, :len(ids)]).tolist() == dist, (what, qi, int(self.slots[qi]))
            assert (oi[qi, len(ids):] == U32_MAX).all() and np.isnan(od[qi, len(ids):]).all(), (what, qi)

    def mixed_call(self, nq, **tun):
        with _lib.tuning(**tun):
            self.index.filter_stats(reset=True)
            got = self.index.search(COUNT, queries=self.queries[:nq], search_k=SK, raw=True, filters=self.filters,
                                    filter_of_query=self.slots[:nq])
            return got, self.index.filter_stats()

    def close(self):
        self.index.close()  # (closes its filters first)
        self.forest.close()
        self.ds.close()


@pytest.fixture(scope="module", params=WORLDS, ids=[w[0] for w in WORLDS])
def world(request):
    _name, metric, ometric, sparse = request.param
    w = World(metric, ometric, sparse)
    yield w
    w.close()


def assert_stats_follow_the_plan(st, slots, group_min, what):
    batches = plan(slots, group_min)
    want = {"calls": 1,
            "uniform_batches": sum(1 for k, _ in batches if k == "uniform"), "mixed_batches": sum(1 for k, _ in batches if k == "mixed"),
            "uniform_queries": sum(b.size for k, b in batches if k == "uniform"), "mixed_queries": sum(b.size for k, b in batches if k == "mixed")}
    assert {k: st[k] for k in want} == want, (what, st)
    return want


def test_mixed_calls_equal_the_oracle_however_they_are_cut(world):
    w = world
    for nq in (1, 5, 64, 700):
        slots = w.slots[:nq]
        got, st = w.mixed_call(nq)
        w.check(got, nq, ("default", nq))
        assert_stats_follow_the_plan(st, slots, _lib.tuning_get("AH_SEARCH_FILTER_GROUP_MIN")[0], nq)
        # all uniform, then all mixed: the same bits, and ah_filter_stats proves which kind of sub-batch ran
        uni, st_u = w.mixed_call(nq, AH_SEARCH_FILTER_GROUP_MIN=1)
        same(uni, got, ("uniform", nq))
        assert st_u["mixed_batches"] == 0 and st_u["uniform_queries"] == nq and st_u["uniform_batches"] == np.unique(slots).size, st_u
        w.index.stats(reset=True)
        mix, st_m = w.mixed_call(nq, AH_SEARCH_FILTER_GROUP_MIN=nq + 1)
        same(mix, got, ("mixed", nq))
        sst = w.index.stats()
        if np.unique(slots).size > 1:
            assert st_m["uniform_batches"] == 0 and st_m["mixed_batches"] == 1 and st_m["mixed_queries"] == nq, st_m
            # a mixed sub-batch never reaches the leaf tiles (they read one visit's kept ids for all visits of a leaf)
            assert sst["rerank_sorted"] == nq and sst["rerank_tiles"] == 0 and sst["tile_visits"] == 0, sst
            assert sst["filtered_queries"] == int((slots != NO_FILTER).sum()) and sst["leaf_kept_passes"] == 0, sst
        else:  # one query: nothing is mixed in it
            assert st_m["uniform_batches"] == 1 and st_m["mixed_batches"] == 0, st_m
        # the wave / block descents of a mixed sub-batch (every filter of it at 5 % or more) against its octet descent
        sub = np.flatnonzero(np.isin(slots, [0, 1, 4, 5, NO_FILTER]))
        if sub.size > 1 and np.unique(slots[sub]).size > 1:
            res = []
            for wave in (1, 0):
                with _lib.tuning(AH_SEARCH_FILTER_GROUP_MIN=nq + 1, AH_SEARCH_WAVE=wave):
                    w.index.stats(reset=True)
                    res.append(w.index.search(COUNT, queries=w.queries[sub], search_k=SK, raw=True, filters=w.filters,
                                              filter_of_query=slots[sub]))
                    sst = w.index.stats()
                    assert w.index.filter_stats()["mixed_batches"] >= 1
                    octet = sst["descent_octet_lds"] + sst["descent_octet_global"]
                    # (1-bit margins are small integers: equal keys of two octets across the cut may leave every query of a
                    # small call to the sequential descent, so the wave side is pinned for the f32 metrics only)
                    if not wave:
                        assert octet == sub.size, (wave, sst)
                    elif w.od.metric < O.BQ_EUCLIDEAN:
                        assert octet < sub.size, (wave, sst)
            same(res[0], res[1], ("wave", nq))
            for x, y in zip(res[0], got):
                assert np.array_equal(bits(x), bits(y[sub])), ("wave vs call", nq)
        # the same queries through ah_search_batch, one call per filter
        for slot in np.unique(slots):
            sel = np.flatnonzero(slots == slot)
            cand = None if slot == NO_FILTER else w.lists[int(slot)]
            one = w.index.search(COUNT, queries=w.queries[sel], search_k=SK, raw=True, candidates=cand, candidates_sorted=True)
            for x, y in zip(one, got):
                assert np.array_equal(bits(x), bits(y[sel])), ("per-filter ah_search_batch", nq, int(slot))
        # the certified screens off, and checked against their bounds
        plain, _ = w.mixed_call(nq, AH_SEARCH_SCREEN=0)
        same(plain, got, ("screen off", nq))
        w.ds.query_screen_verify(reset=True)
        ver, _ = w.mixed_call(nq, AH_SCREEN_VERIFY=1)
        same(ver, got, ("verify", nq))
        assert w.ds.query_screen_verify()["violations"] == 0


def test_by_item_queries_and_the_default_slot_rules(world):
    w = world
    items = w.ids[[3, N - 1, 1234, 777, 31_000, 9]]
    slots = np.array([1, 0, NO_FILTER, 0, 4, 2], dtype=np.uint32)
    got = w.index.search(COUNT, items=items, search_k=SK, raw=True, filters=w.filters, filter_of_query=slots)
    for qi in range(len(items)):
        cand = None if slots[qi] == NO_FILTER else w.lists[int(slots[qi])]
        one = w.index.search(COUNT, items=items[qi:qi + 1], search_k=SK, raw=True, candidates=cand, candidates_sorted=True)
        for x, y in zip(one, got):
            assert np.array_equal(bits(x[0]), bits(y[qi])), qi
    # filter_of_query = NULL: every query under filters[0], or unfiltered without filters; a Filter as `candidates`
    a = w.index.search(COUNT, queries=w.queries[:9], search_k=SK, raw=True, filters=[w.filters[1]])
    b = w.index.search(COUNT, queries=w.queries[:9], search_k=SK, raw=True, candidates=w.lists[1], candidates_sorted=True)
    same(a, b)
    same(w.index.search(COUNT, queries=w.queries[:9], search_k=SK, raw=True, candidates=w.filters[1]), b)
    same(w.index.search(COUNT, queries=w.queries[:9], search_k=SK, raw=True, filters=[]),
         w.index.search(COUNT, queries=w.queries[:9], search_k=SK, raw=True))


def test_resident_filter_uniform_calls(world):
    w = world
    f = w.filters[0]
    qs = np.flatnonzero(w.slots == 0)[:50]
    assert qs.size == 50
    w.index.stats(reset=True)
    w.index.filter_stats(reset=True)
    for qi in qs:  # one query per call, arroy's API shape
        got = w.index.search(COUNT, queries=w.queries[qi:qi + 1], search_k=SK, raw=True, filters=[f])
        ids, dist = w.truth(int(qi))
        assert got[0][0, :got[2][0]].tolist() == ids and bits(got[1][0, :got[2][0]]).tolist() == dist, qi
    st, fst = w.index.stats(), w.index.filter_stats()
    assert st["leaf_kept_passes"] == 0 and fst["leaf_kept_passes"] == 0 and st["calls"] == 50 and st["filtered_queries"] == 50, (st, fst)
    assert fst["uniform_batches"] == 50 and fst["mixed_batches"] == 0, fst
    # the block / multi descent served them, not the sequential one that a call too small for its own pass over the forest takes
    # (1-bit distances are small integers: equal keys of two octets across the cut are common there and legitimately leave a
    # query to the sequential descent, so the counters are pinned for the f32 metrics)
    if w.od.metric < O.BQ_EUCLIDEAN:
        assert st["descent_block"] == 50 and st["descent_octet_lds"] + st["descent_octet_global"] == 0, st
    # the same filter from four threads at once
    want = w.index.search(COUNT, queries=w.queries[qs], search_k=SK, raw=True, filters=[f])
    out, errs = [None] * 4, []

    def worker(t):
        try:
            res = []
            for _ in range(5):
                res.append(w.index.search(COUNT, queries=w.queries[qs[t::4]], search_k=SK, raw=True, filters=[f]))
            out[t] = res
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for t in range(4):
        for res in out[t]:
            for x, y in zip(res, want):
                assert np.array_equal(bits(x), bits(y[t::4])), t


def test_filter_lifetime_info_and_refusals(world):
    w = world
    L = _lib.lib()
    # ah_filter_info: listed, stored (exact, also on sparse ids), bytes held
    stored_set = set(w.ids.tolist())
    for lst, f in zip(w.lists, w.filters):
        info = f.info()
        assert info["listed"] == lst.size and info["stored"] == sum(1 for i in lst.tolist() if i in stored_set), info
        n_nodes = int(w.view.n_nodes)
        assert info["device_bytes"] >= n_nodes * 4 + (int(w.ids[-1]) + 1) // 8, info
    with pytest.raises(_lib.ArroyHipError, match="strictly ascending"):
        w.index.make_filter(np.array([5, 4, 9], dtype=np.uint32), sorted=True)
    with pytest.raises(_lib.ArroyHipError, match="strictly ascending"):
        w.index.make_filter(np.array([5, 5, 9], dtype=np.uint32), sorted=True)
    # live bytes return to their earlier value after destroy (a first filter warms the calling thread's context up)
    w.index.make_filter(w.lists[0], sorted=True).close()
    live0, _ = _lib.device_cache_stats(w.ds.device)
    st0 = w.index.filter_stats()
    f = w.index.make_filter(w.lists[1], sorted=True)
    live1, _ = _lib.device_cache_stats(w.ds.device)
    st1 = w.index.filter_stats()
    assert live1 - live0 == f.info()["device_bytes"], (live0, live1, f.info())
    assert st1["filters_alive"] == st0["filters_alive"] + 1 and st1["filters_created"] == st0["filters_created"] + 1
    assert st1["leaf_kept_passes"] == st0["leaf_kept_passes"] + 1
    f.close()
    assert _lib.device_cache_stats(w.ds.device)[0] == live0
    assert w.index.filter_stats()["filters_alive"] == st0["filters_alive"]
    # a filter of another index; ah_index_destroy with a live filter
    other = Index(w.ds, w.forest)
    try:
        fo = other.make_filter(w.lists[0], sorted=True)
        with pytest.raises(_lib.ArroyHipError, match="another index"):
            w.index.search(COUNT, queries=w.queries[:2], search_k=SK, raw=True, filters=[w.filters[0], fo],
                           filter_of_query=[0, 1])
        assert L.ah_index_destroy(other._h) == 5 and b"live filter" in L.ah_last_error()
        same(other.search(COUNT, queries=w.queries[:3], search_k=SK, raw=True, filters=[fo]),  # ... and it still works
             w.index.search(COUNT, queries=w.queries[:3], search_k=SK, raw=True, filters=[w.filters[0]]))
        fo.close()
        assert L.ah_index_destroy(other._h) == 0
        other._h = type(other._h)()
    finally:
        other.close()


def sweep_once(op, cleanup, limit=2000):
    """tests/test_gpu_faults.py: op() with the n-th allocation failing, n = 1, 2, ... until a call has no n-th allocation."""
    seen = []
    for n in range(1, limit):
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", n)
        try:
            res, status = op(), OK
        except _lib.ArroyHipError as e:
            res, status = None, e.status
        finally:
            left = _lib.tuning_get("AH_FAIL_ALLOC_AFTER")[0]
            _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        assert status in (OK, DEVICE, OOM), (n, status)
        if status != OK:
            assert _lib.lib().ah_last_error() != b"", n
        if res is not None and cleanup is not None:
            cleanup(res)
        if left > 0:
            assert status == OK
            return seen
        seen.append(status)
    raise AssertionError(f"more than {limit} allocations in one call?")


def sweep(op, cleanup=None):
    seen = sweep_once(op, cleanup)
    live1, _ = _lib.device_cache_stats(0)
    again = sweep_once(op, cleanup)
    live2, _ = _lib.device_cache_stats(0)
    assert live2 <= live1, f"{len(again)} failing calls leaked {live2 - live1} bytes of HBM"
    return seen


def test_filter_create_and_batched_search_survive_every_allocation_failure():
    """Injected allocation failures return a status by design (they are not device faults): every allocation of
    ah_filter_create and of ah_search_batch_filters fails once, and the next call gives the right bits."""
    w = World(D.Cosine, O.COSINE, False)
    try:
        alive = w.index.filter_stats()["filters_alive"]
        seen = sweep(lambda: w.index.make_filter(w.lists[1], sorted=True), cleanup=lambda f: f.close())
        assert len(seen) >= 3 and OOM in seen, seen  # the handle, the filter's block, the list's staging block
        assert w.index.filter_stats()["filters_alive"] == alive  # a failure leaves nothing behind
        nq = 700
        want, _ = w.mixed_call(nq)
        for gmin in (16, nq + 1):
            # (a warmed-up search allocates nothing on the device: every sweep submits more queries than any call before it)
            big = np.concatenate([w.queries] * (2 if gmin == 16 else 4))
            bslots = np.concatenate([w.slots] * (2 if gmin == 16 else 4))
            with _lib.tuning(AH_SEARCH_FILTER_GROUP_MIN=gmin):
                seen = sweep(lambda: w.index.search(COUNT, queries=big, search_k=SK, raw=True, filters=w.filters, filter_of_query=bslots))
                assert len(seen) >= 4 and all(s in (OOM, DEVICE) for s in seen), (gmin, seen)  # host vectors at the least
                got, _ = w.mixed_call(nq)
            same(got, want, gmin)
        w.check(want, nq, "after the sweeps")
    finally:
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        w.close()


def test_one_larger_case_1m_x_768_cosine_20_trees_8_filters():
    n, dims, trees, count, sk, nq = 1_000_000, 768, 20, 100, 10_000, 1000
    ds = Dataset(D.Cosine, dims, n)
    ds.fill_synthetic(42, 1, n)
    ds.finalize()
    forest = ds.build_forest(shard.tree_seeds(42, range(trees)))
    index = ds.create_index(forest)
    try:
        rng = np.random.default_rng(8)
        vecs = O.synth(42, 1, n, dims)
        queries = (vecs[rng.choice(n, nq, replace=False)] + rng.standard_normal((nq, dims)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
        ids = np.arange(n, dtype=np.uint32)
        lists = [ids[::2].copy(), ids[1::3].copy(), ids[::10].copy(), ids[::20].copy(), ids[::100].copy(), ids[::1000].copy(),
                 ids[:n // 4].copy(), np.sort(rng.choice(n, n // 7, replace=False)).astype(np.uint32)]
        filters = [index.make_filter(x, sorted=True) for x in lists]
        # slots of very different popularity: long runs (uniform sub-batches) and short ones (mixed) in one call
        p = np.array([0.3, 0.25, 0.2, 0.1, 0.01, 0.01, 0.008, 0.005, 0.117])
        slots = rng.choice(9, nq, p=p / p.sum()).astype(np.uint32)
        slots[slots == 8] = NO_FILTER
        index.filter_stats(reset=True)
        got = index.search(count, queries=queries, search_k=sk, raw=True, filters=filters, filter_of_query=slots)
        st = index.filter_stats()
        assert_stats_follow_the_plan(st, slots, _lib.tuning_get("AH_SEARCH_FILTER_GROUP_MIN")[0], "large")
        assert st["uniform_batches"] >= 1 and st["mixed_batches"] >= 1, st
        with _lib.tuning(AH_SEARCH_FILTER_GROUP_MIN=nq + 1):
            same(index.search(count, queries=queries, search_k=sk, raw=True, filters=filters, filter_of_query=slots), got, "all mixed")
        for slot in np.unique(slots):  # per-filter ah_search_batch calls: every query
            sel = np.flatnonzero(slots == slot)
            cand = None if slot == NO_FILTER else lists[int(slot)]
            one = index.search(count, queries=queries[sel], search_k=sk, raw=True, candidates=cand, candidates_sorted=True)
            for x, y in zip(one, got):
                assert np.array_equal(bits(x), bits(y[sel])), int(slot)
        od = O.Data(O.COSINE, vecs)
        view = O.forest_view(forest)
        for qi in rng.choice(nq, 40, replace=False):  # the oracle: a sample
            qv, qh = od.query_leaf(queries[qi])
            cand = None if slots[qi] == NO_FILTER else lists[int(slots[qi])]
            want, _ = O.search(od, forest, qv, qh, count, sk, 0, cand, candidates_sorted=True, want_candidates=False, view=view)
            assert int(got[2][qi]) == len(want) and got[0][qi, :len(want)].tolist() == [i for i, _ in want], qi
            assert bits(got[1][qi, :len(want)]).tolist() == np.array([d for _, d in want], dtype=np.float32).view(np.uint32).tolist(), qi
    finally:
        index.close()
        forest.close()
        ds.close()
