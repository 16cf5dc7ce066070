"""Exhausted filters (AH_SEARCH_EXHAUSTED=1): a query whose resident filter keeps at most its effective search_k ids over all
leaves is answered from the filter's kept list K(f), without the descent — the reference's ids and distance bits.

The truth is always the oracle (`O.search` under the filter's id list) or numpy on the index's exported arrays, never the
library; ah_exhausted_stats proves that the new path ran (a silent fall-back to the descent fails the tests), and the cut of
every call is held against plan_exhausted (tests/test_search_exhausted_cpu.py)."""
import threading

import numpy as np
import pytest

from arroy_amd import Dataset, _lib, shard
from arroy_amd import distances as D
from oracle import oracle as O
from test_gpu_search_filters import sweep
from test_search_exhausted_cpu import plan_exhausted, stats_of_plan
from test_search_filters_cpu import NO_FILTER

pytestmark = pytest.mark.gpu

N, DIMS, TREES = 20_000, 96, 12
COUNT, SK = 25, 1500
U32_MAX = 0xFFFFFFFF
SLAB = 64                      # batch.hip: kSharedSlab, the list rows of one block of k_shared_list_distances
GROUP = 16                     # batch.hip: kSharedGroup, the queries of one block
EDGE_DIMS = (3, 40, 65, 130)   # below a line of 32, a line and a tail, two lines and one element, four lines and a tail
ON = dict(AH_SEARCH_EXHAUSTED=1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what=""):
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y)), what


class World:
    def __init__(self, metric, ometric, sparse=False, n=N, dims=DIMS, trees=TREES, vecs=None, nq=700, seed=7):
        vecs = O.synth(seed, 2, n, dims) if vecs is None else vecs
        if sparse:  # ascending ids with gaps, the last one u32::MAX (src/tests/writer.rs:161-179)
            ids = (np.arange(n, dtype=np.uint64) * 3 + (np.arange(n, dtype=np.uint64) % 2)).astype(np.uint32)
            ids[-1] = U32_MAX
        else:
            ids = np.arange(n, dtype=np.uint32)
        self.n, self.dims, self.trees, self.ids, self.vecs = n, dims, trees, ids, vecs
        self.ds = Dataset(metric, dims, n)
        self.ds.upload_vectors(ids, vecs)
        self.od = O.Data(ometric, vecs, ids=ids if sparse else None)
        if metric is D.DotProduct:
            self.ds.preprocess_dot()
            self.od.preprocess_dot()
        self.ds.finalize()
        self.forest = self.ds.build_forest(shard.tree_seeds(seed, range(trees)))
        self.index = self.ds.create_index(self.forest)
        self.view = O.forest_view(self.forest)
        rng = np.random.default_rng(3)
        self.queries = (vecs[rng.choice(n, nq)] + rng.standard_normal((nq, dims)).astype(np.float32) * np.float32(0.1)).astype(np.float32)
        self.leaf_ids = self.read_leaf_ids()
        self.desc_len = self.leaf_ids.size
        top = int(ids[-1])
        if top < U32_MAX - 100:
            tail = np.arange(top + 1, top + 60, 3, dtype=np.uint32)
            absent = np.arange(top + 2, top + 90, 2, dtype=np.uint32)
        else:  # the gaps between the stored ids
            gaps = np.setdiff1d(np.arange(0, 3000, dtype=np.uint32), ids)
            tail, absent = gaps[::2].astype(np.uint32), gaps[1::2].astype(np.uint32)
        step = max(1, n // 100)
        self.lists = {"strided": ids[::step][:100].copy(), "empty": np.zeros(0, np.uint32), "all": ids.copy(),
                      "tail": np.union1d(ids[1::step][:90], tail).astype(np.uint32), "absent": absent,
                      "x125": ids[3::max(1, n // 130)][:125].copy(), "x126": ids[5::max(1, n // 130)][:126].copy(),
                      "half": ids[::2].copy()}
        self.names = list(self.lists)
        self.filters = {k: self.index.make_filter(v, sorted=True) for k, v in self.lists.items()}
        self._truth = {}

    def read_leaf_ids(self):
        """The ids of every in-use leaf, leaf after leaf, from the index's exported arrays."""
        ex = self.index.export(normals=False)
        nodes, desc = ex["nodes"], ex["descendants"]
        leaves = np.flatnonzero((nodes["kind"] == 1) & (nodes["count"] > 0))
        return np.concatenate([desc[int(nodes["offset"][i]):int(nodes["offset"][i]) + int(nodes["count"][i])] for i in leaves]
                              + [np.zeros(0, np.uint32)])

    def kept_total(self, lst):
        return int(np.isin(self.leaf_ids, lst).sum())

    def kept_ids(self, lst):
        return np.intersect1d(lst, self.leaf_ids).astype(np.uint32)

    def truth(self, key, leaf, lst, count=COUNT, sk=SK):
        """(ids, distance bits) by the oracle; `leaf` = (vector, header) of the query, `key` names it for the cache."""
        key = (key, None if lst is None else hash(lst.tobytes()), count, sk)
        if key not in self._truth:
            want, _ = O.search(self.od, self.forest, leaf[0], leaf[1], count, sk, 1, lst, candidates_sorted=True, want_candidates=False,
                               view=self.view)
            self._truth[key] = ([i for i, _ in want], np.array([d for _, d in want], dtype=np.float32).view(np.uint32).tolist())
        return self._truth[key]

    def check_row(self, got, row, want, what, any_nan_sign=False):
        """any_nan_sign: every NaN compares as 0x7FC00000 — the sign of the NaN an invalid operation makes is the platform's
        (tests/test_gpu_query_screens.py: canonical_nan), so the oracle's differs from the device's where a row holds one."""
        oi, od, oc = got
        ids, dist = want
        assert int(oc[row]) == len(ids), (what, row, int(oc[row]), len(ids))
        assert oi[row, :len(ids)].tolist() == ids, (what, row)
        have = bits(od[row, :len(ids)]).copy()
        if any_nan_sign:
            have[np.isnan(od[row, :len(ids)])] = 0x7FC00000
            dist = [0x7FC00000 if (d & 0x7FFFFFFF) > 0x7F800000 else d for d in dist]
        assert have.tolist() == dist, (what, row)
        assert (oi[row, len(ids):] == U32_MAX).all() and np.isnan(od[row, len(ids):]).all(), (what, row)

    def check(self, got, qis, slot_names, what, count=COUNT, sk=SK):
        for row, (qi, name) in enumerate(zip(qis, slot_names)):
            lst = None if name is None else self.lists[name]
            self.check_row(got, row, self.truth(int(qi), self.od.query_leaf(self.queries[qi]), lst, count, sk), (what, name))

    def search(self, qis, names, slot_names, **tun):
        """One ah_search_batch_filters call over queries `qis`, query i under filter names[slot] for slot_names[i] (None: no filter)."""
        slots = np.array([NO_FILTER if s is None else names.index(s) for s in slot_names], dtype=np.uint32)
        with _lib.tuning(**tun):
            return self.index.search(COUNT, queries=self.queries[qis], search_k=SK, oversampling=1, raw=True,
                                     filters=[self.filters[k] for k in names], filter_of_query=slots)

    def reset_stats(self):
        self.index.exhausted_stats(reset=True)
        self.index.filter_stats(reset=True)
        self.index.stats(reset=True)
        self.index.params_stats(reset=True)

    def close(self):
        self.index.close()  # (closes its filters first)
        self.forest.close()
        self.ds.close()


WORLDS = {"cosine": (D.Cosine, O.COSINE, False), "dot": (D.DotProduct, O.DOT_PRODUCT, False), "euclidean": (D.Euclidean, O.EUCLIDEAN, False),
          "manhattan": (D.Manhattan, O.MANHATTAN, False), "bq_cosine": (D.BinaryQuantizedCosine, O.BQ_COSINE, False),
          "euclidean_sparse_ids": (D.Euclidean, O.EUCLIDEAN, True)}


@pytest.fixture(scope="module", params=list(WORLDS), ids=list(WORLDS))
def world(request):
    w = World(*WORLDS[request.param])
    yield w
    w.close()


# ---- 1. totals and lists ---------------------------------------------------------------------------------------------------

def test_kept_total_and_kept_ids_are_numpy_on_the_forest(world):
    w = world
    for name in ("strided", "empty", "all", "tail", "absent", "x125"):
        f, lst = w.filters[name], w.lists[name]
        assert f.kept_total() == w.kept_total(lst), name
        assert np.array_equal(f.kept_ids(), w.kept_ids(lst)), name
        assert f.kept_total() == f.kept_total() and np.array_equal(f.kept_ids(), f.kept_ids()), name  # (cached: the same again)
    assert w.filters["x125"].kept_total() == 125 * TREES and w.filters["absent"].kept_ids().size == 0
    # a combined filter and a bitmap-made one
    both = w.filters["half"] & w.filters["strided"]
    want = np.intersect1d(w.lists["half"], w.lists["strided"])
    assert want.size and both.kept_total() == w.kept_total(want) and np.array_equal(both.kept_ids(), w.kept_ids(want))
    both.close()
    n_bits = int(min(int(w.ids[-1]) + 1, 5000))
    sel = w.lists["tail"][w.lists["tail"] < n_bits]
    words = np.zeros((n_bits + 63) // 64, dtype=np.uint64)
    np.bitwise_or.at(words, (sel >> 6).astype(np.int64), np.uint64(1) << (sel & 63).astype(np.uint64))
    fb = w.index.make_filter_bitmap(words, n_bits)
    assert fb.kept_total() == w.kept_total(sel) and np.array_equal(fb.kept_ids(), w.kept_ids(sel))
    fb.close()


def test_totals_and_lists_after_suspend_delete_and_resume():
    w = World(D.Euclidean, O.EUCLIDEAN, n=2000, dims=40, trees=5, nq=4)
    try:
        lst = w.ids[::7].copy()
        f = w.index.make_filter(lst, sorted=True)
        assert np.array_equal(f.kept_ids(), lst) and f.kept_total() == lst.size * 5
        bytes_with_list = f.info()["device_bytes"]
        for g in w.filters.values():
            g.close()
        f.suspend()
        assert f.info()["device_bytes"] < bytes_with_list  # the list went with the per-node counts it was made from
        with pytest.raises(_lib.ArroyHipError, match="suspended"):
            f.kept_total()
        with pytest.raises(_lib.ArroyHipError, match="suspended"):
            f.kept_ids()
        gone = np.union1d(lst[::3], w.ids[1::50]).astype(np.uint32)
        w.index.delete_items(gone, w.dims)  # (the bound the forest was built with: split_after 0 = dimensions)
        w.index.exhausted_stats(reset=True)
        w.index.resume_filters([f], [(gone, None)])
        w.leaf_ids = w.read_leaf_ids()
        left = np.setdiff1d(lst, gone).astype(np.uint32)
        assert not np.isin(gone, w.leaf_ids).any()
        assert w.index.exhausted_stats()["lists_made"] == 0  # lazily: the resume made nothing
        assert f.kept_total() == w.kept_total(left) == left.size * 5
        assert np.array_equal(f.kept_ids(), left) and w.index.exhausted_stats()["lists_made"] == 1
        # a filter that still lists the deleted ids: they are in its bitmap, and in no leaf
        stale = w.index.make_filter(lst, sorted=True)
        assert stale.kept_total() == w.kept_total(lst) == left.size * 5 and np.array_equal(stale.kept_ids(), left)
    finally:
        w.close()


# ---- 2. the boundary -------------------------------------------------------------------------------------------------------

def test_the_boundary_125_ids_fit_search_k_1500_and_126_do_not(world):
    w = world
    assert w.kept_total(w.lists["x125"]) == SK and w.kept_total(w.lists["x126"]) == SK + TREES
    qis = np.arange(20)
    for name, exhausted in (("x125", True), ("x126", False)):
        off = w.search(qis, [name], [name] * 20)
        w.reset_stats()
        on = w.search(qis, [name], [name] * 20, **ON)
        xs, ss, fs = w.index.exhausted_stats(), w.index.stats(), w.index.filter_stats()
        same(on, off, name)
        w.check(on, qis, [name] * 20, "boundary")
        if exhausted:
            assert (xs["queries"], xs["batches"], xs["empty_queries"]) == (20, 1, 0), xs
            assert ss["queries"] == 0 and ss["chunks"] == 0 and ss["calls"] == 1 and fs["uniform_batches"] + fs["mixed_batches"] == 0, (ss, fs)
        else:
            assert xs["queries"] == 0 and xs["batches"] == 0 and ss["queries"] == 20 and fs["uniform_queries"] == 20, (xs, ss, fs)
        assert fs["calls"] == 1


# ---- 3. a mixed call -------------------------------------------------------------------------------------------------------

def test_a_mixed_call_follows_the_plan_and_equals_the_oracle(world):
    w = world
    names = ["strided", "x126", "absent", "x125", "half", "tail", "all", "empty"]
    rng = np.random.default_rng(12)
    nq = 700
    slots = rng.integers(0, len(names) + 1, nq)
    slot_names = [None if s == len(names) else names[s] for s in slots]
    u32 = np.array([NO_FILTER if s is None else names.index(s) for s in slot_names], dtype=np.uint32)
    qis = np.arange(nq)
    kept = np.array([w.kept_total(w.lists[k]) for k in names])
    lens = np.array([w.kept_ids(w.lists[k]).size for k in names])
    for gmin in (16, 701):
        off = w.search(qis, names, slot_names, AH_SEARCH_FILTER_GROUP_MIN=gmin)
        w.reset_stats()
        on = w.search(qis, names, slot_names, AH_SEARCH_FILTER_GROUP_MIN=gmin, **ON)
        xs, fs, ss = w.index.exhausted_stats(), w.index.filter_stats(), w.index.stats()
        same(on, off, gmin)
        p = plan_exhausted(u32, kept, min(SK, w.desc_len), COUNT, gmin, list_lens=lens)
        want_xs, want_fs, want_ss, _ = stats_of_plan(p, COUNT, SK, params=False)
        assert want_xs["queries"] > 200 and want_xs["empty_queries"] > 50 and len(p["rest"]) >= 1
        assert {k: xs[k] for k in want_xs} == want_xs, (gmin, xs, want_xs)
        assert {k: fs[k] for k in want_fs} == want_fs, (gmin, fs, want_fs)
        assert {k: ss[k] for k in want_ss} == want_ss, (gmin, ss, want_ss)
        descents = ("descent_wave_small", "descent_wave_big", "descent_octet_lds", "descent_octet_global", "descent_block", "descent_multi")
        assert sum(ss[k] for k in descents if k in ss) >= ss["queries"] == p["live"].size, ss
    w.check(on, qis, slot_names, "mixed call")


# ---- 4. ah_search_batch_params ---------------------------------------------------------------------------------------------

def test_per_query_search_k_straddles_kept_total_and_counts_straddle_the_list(world):
    w = world
    name = "strided"
    f, lst = w.filters[name], w.lists[name]
    total, m = w.kept_total(lst), w.kept_ids(lst).size
    assert m == 100 and total == m * TREES
    sks = np.array([total - 1, total, total + 1, 10 ** 6, total, total, total, total, 5], dtype=np.uint64)
    counts = np.array([10, 10, 10, 10, 1, m - 1, m, m + 5, m + 5], dtype=np.uint32)
    qis = np.arange(sks.size)
    kw = dict(queries=w.queries[qis], search_ks=sks, oversamplings=1, filters=[f], raw=True)
    off = w.index.search_params(counts, **kw)
    w.reset_stats()
    with _lib.tuning(**ON):
        on = w.index.search_params(counts, **kw)
    xs, ps, ss = w.index.exhausted_stats(), w.index.params_stats(), w.index.stats()
    same(on, off, "params")
    assert on[0].shape == (sks.size, m + 5)
    for row in range(sks.size):
        want = w.truth(int(qis[row]), w.od.query_leaf(w.queries[row]), lst, int(counts[row]), int(sks[row]))
        w.check_row(on, row, want, "params")
    assert on[2][4:8].tolist() == [1, m - 1, m, m]  # out_counts = min(count, m), the padding intact behind it (check_row)
    assert (xs["queries"], xs["batches"], xs["empty_queries"]) == (7, 1, 0), xs
    assert ps["calls"] == 1 and ps["queries"] == sks.size and ps["batches"] == ss["chunks"] and ss["queries"] == 2, (ps, ss)


def test_an_effective_count_beyond_the_batched_top_k_goes_query_by_query():
    w = World(D.Cosine, O.COSINE, n=8000, dims=40, trees=12, nq=3)
    try:
        lst = w.ids[::3][:2100].copy()
        f = w.index.make_filter(lst, sorted=True)
        assert w.kept_total(lst) == 25_200 and w.kept_ids(lst).size == 2100
        counts, sks = np.array([3000, 2048, 3000], dtype=np.uint32), np.array([25_200, 30_000, 25_199], dtype=np.uint64)
        kw = dict(queries=w.queries[:3], search_ks=sks, oversamplings=1, filters=[f], raw=True)
        off = w.index.search_params(counts, **kw)
        w.reset_stats()
        with _lib.tuning(**ON):
            on = w.index.search_params(counts, **kw)
        xs, ps = w.index.exhausted_stats(), w.index.params_stats()
        same(on, off, "big count")
        for row in range(3):
            w.check_row(on, row, w.truth(row, w.od.query_leaf(w.queries[row]), lst, int(counts[row]), int(sks[row])), "big count")
        assert on[2].tolist() == [2100, 2048, 2100]
        # two exhausted sub-batches: effective count 2048 (batched top-k), effective count 2100 (the single-query kernel)
        assert (xs["queries"], xs["batches"]) == (2, 2) and ps["big_count_queries"] == 1 and ps["batches"] == 1, (xs, ps)
    finally:
        w.close()


# ---- 5. by-item queries ----------------------------------------------------------------------------------------------------

def test_by_item_queries_inside_and_outside_the_filter(world):
    w = world
    lst = w.lists["x125"]
    inside, outside = int(np.flatnonzero(w.ids == lst[7])[0]), int(np.flatnonzero(~np.isin(w.ids, lst))[11])
    items = w.ids[[inside, outside]]
    off = w.index.search(COUNT, items=items, search_k=SK, oversampling=1, raw=True, filters=[w.filters["x125"]])
    w.reset_stats()
    with _lib.tuning(**ON):
        on = w.index.search(COUNT, items=items, search_k=SK, oversampling=1, raw=True, filters=[w.filters["x125"]])
    same(on, off, "by item")
    assert w.index.exhausted_stats()["queries"] == 2
    for row, r in enumerate((inside, outside)):
        w.check_row(on, row, w.truth(("item", r), w.od.item_leaf(r), lst), "by item")
    if w.od.metric != O.DOT_PRODUCT:  # itself, at distance 0 (equal distances: by id)
        assert int(lst[7]) in on[0][0].tolist()


# ---- 6. non-finite rows ----------------------------------------------------------------------------------------------------

def test_non_finite_rows_follow_the_positional_rule():
    n, dims = 2000, 32
    rng = np.random.default_rng(9)
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    vecs[5, 3] = np.float32(np.inf)
    vecs[700, [1, 9]] = np.float32(np.nan)
    vecs[1500, 30] = -np.float32(np.inf)
    w = World(D.Euclidean, O.EUCLIDEAN, n=n, dims=dims, trees=8, vecs=vecs, nq=6)
    try:
        lst = np.union1d(w.ids[::40], [5, 700, 1500]).astype(np.uint32)
        f = w.index.make_filter(lst, sorted=True)
        for count in (1, 2, 10, lst.size):
            kw = dict(queries=w.queries, search_k=10_000, oversampling=1, raw=True, filters=[f])
            off = w.index.search(count, **kw)
            w.reset_stats()
            with _lib.tuning(**ON):
                on = w.index.search(count, **kw)
            same(on, off, count)
            assert w.index.exhausted_stats()["queries"] == 6
            for row in range(6):
                w.check_row(on, row, w.truth(row, w.od.query_leaf(w.queries[row]), lst, count, 10_000), ("non-finite", count),
                            any_nan_sign=True)
    finally:
        w.close()


# ---- 7. the kernels' edges -------------------------------------------------------------------------------------------------

EDGE_METRICS = {"euclidean": (D.Euclidean, O.EUCLIDEAN), "cosine": (D.Cosine, O.COSINE), "manhattan": (D.Manhattan, O.MANHATTAN),
                "dot": (D.DotProduct, O.DOT_PRODUCT), "bq_cosine": (D.BinaryQuantizedCosine, O.BQ_COSINE),
                "bq_euclidean": (D.BinaryQuantizedEuclidean, O.BQ_EUCLIDEAN)}


@pytest.mark.parametrize("dims", EDGE_DIMS)
@pytest.mark.parametrize("metric", list(EDGE_METRICS))
def test_list_lengths_around_the_slab_and_calls_around_the_query_group(metric, dims):
    w = World(*EDGE_METRICS[metric], n=2000, dims=dims, trees=3, nq=2 * GROUP + 1, seed=dims)
    try:
        sk = 10_000  # (clamped to the 6000 ids of the forest: every list below fits)
        calls = [(m, 2 * GROUP + 1) for m in (1, 7, 8, 9, SLAB - 1, SLAB, SLAB + 1)] + \
                [(m, nq) for m in (9, 2 * SLAB + 1) for nq in (1, GROUP - 1, GROUP, GROUP + 1)]
        made = {}
        w.reset_stats()
        for m, nq in calls:
            if m not in made:
                lst = w.ids[m % 5::11][:m].copy()
                made[m] = (lst, w.index.make_filter(lst, sorted=True))
            lst, f = made[m]
            assert lst.size == m
            with _lib.tuning(**ON):
                on = w.index.search(COUNT, queries=w.queries[:nq], search_k=sk, oversampling=1, raw=True, filters=[f])
            for row in range(nq):
                w.check_row(on, row, w.truth(row, w.od.query_leaf(w.queries[row]), lst, COUNT, sk), (metric, dims, m, nq))
        xs = w.index.exhausted_stats()
        assert xs["queries"] == sum(nq for _m, nq in calls) and xs["batches"] == len(calls) and xs["lists_made"] == len(made), xs
    finally:
        w.close()


# ---- 8. empty lists --------------------------------------------------------------------------------------------------------

def test_a_filter_that_keeps_nothing_stored_is_answered_without_a_launch_or_a_list(world):
    w = world
    for name in ("absent", "empty"):
        f = w.filters[name]
        b0 = f.info()["device_bytes"]
        w.reset_stats()
        on = w.search(np.arange(9), [name], [name] * 9, **ON)
        xs, ss = w.index.exhausted_stats(), w.index.stats()
        assert (on[2] == 0).all() and (on[0] == U32_MAX).all() and np.isnan(on[1]).all()
        assert (xs["queries"], xs["empty_queries"], xs["batches"], xs["lists_made"], xs["list_ids"]) == (9, 9, 0, 0, 0), xs
        assert ss["queries"] == 0 and ss["chunks"] == 0 and f.info()["device_bytes"] == b0
        same(on, w.search(np.arange(9), [name], [name] * 9), name)


# ---- 9. first use from four threads at once --------------------------------------------------------------------------------

def test_first_use_from_four_threads_makes_one_list(world):
    w = world
    lst = w.ids[11::211][:90].copy()
    f = w.index.make_filter(lst, sorted=True)
    qis = np.arange(40)
    w.reset_stats()
    out, errs = [None] * 4, []
    gate = threading.Barrier(4)

    def worker(t):
        try:
            gate.wait()
            out[t] = w.index.search(COUNT, queries=w.queries[qis], search_k=SK, oversampling=1, raw=True, filters=[f])
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    with _lib.tuning(**ON):
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errs, errs
    xs = w.index.exhausted_stats()
    assert xs["lists_made"] == 1 and xs["list_ids"] == 90 and xs["queries"] == 160 and xs["batches"] == 4, xs
    for t in range(1, 4):
        same(out[t], out[0], t)
    for row in qis:
        w.check_row(out[0], int(row), w.truth(int(row), w.od.query_leaf(w.queries[row]), lst), "threads")
    f.close()


# ---- 10. allocation failures -----------------------------------------------------------------------------------------------

def test_an_exhausted_call_with_list_creation_survives_every_allocation_failure():
    """Injected allocation failures return a status by design (they are not device faults): every allocation of a filter's
    creation and of the exhausted call that makes its list fails once; no list is left half made, no HBM leaks, and the next
    call gives the right bits."""
    w = World(D.Cosine, O.COSINE, n=4000, dims=40, trees=6, nq=40)
    try:
        lst = w.ids[5::37][:100].copy()
        nq = 40
        slots = np.array([0, NO_FILTER] * (nq // 2), dtype=np.uint32)

        def op():
            # (a fresh filter a call: its block, its staged id list, then the scratch and the block of its kept list are device
            # allocations of every call, however warm the context's own scratch is)
            f = w.index.make_filter(lst, sorted=True)
            b0 = f.info()["device_bytes"]
            w.index.exhausted_stats(reset=True)
            try:
                return w.index.search(COUNT, queries=w.queries, search_k=SK, oversampling=1, raw=True, filters=[f], filter_of_query=slots)
            finally:
                made, has = w.index.exhausted_stats()["lists_made"], f.info()["device_bytes"] > b0
                f.close()
                assert made == int(has), (made, has)
        with _lib.tuning(**ON):
            seen = sweep(op)
            assert len(seen) >= 6 and 4 in seen, seen  # the handle, the blocks, the host vectors, the list's scratch and block
            f = w.index.make_filter(lst, sorted=True)
            w.reset_stats()
            got = w.index.search(COUNT, queries=w.queries, search_k=SK, oversampling=1, raw=True, filters=[f], filter_of_query=slots)
            assert w.index.exhausted_stats()["queries"] == nq // 2
        for row in range(nq):
            w.check_row(got, row, w.truth(row, w.od.query_leaf(w.queries[row]), lst if slots[row] == 0 else None), "after the sweeps")
    finally:
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        w.close()


# ---- 11. lifetime and the default ------------------------------------------------------------------------------------------

def test_the_list_is_accounted_for_and_the_default_makes_nothing(world):
    w = world
    assert _lib.tuning_get("AH_SEARCH_EXHAUSTED")[0] == 0
    lst = w.lists["x125"]
    w.index.make_filter(lst, sorted=True).kept_ids()  # (warms the calling thread's context up; closed with the index)
    f = w.index.make_filter(lst, sorted=True)
    # the default: a filtered call over an exhausted filter moves none of the new counters and makes no list
    w.reset_stats()
    b0 = f.info()["device_bytes"]
    off = w.index.search(COUNT, queries=w.queries[:5], search_k=SK, oversampling=1, raw=True, filters=[f])
    xs = w.index.exhausted_stats()
    assert all(v == 0 for v in xs.values()) and f.info()["device_bytes"] == b0 and w.index.stats()["queries"] == 5, xs
    # the list's block: in device_bytes from the moment it exists, gone from the allocator's live bytes at destroy
    live0, _ = _lib.device_cache_stats(w.ds.device)
    with _lib.tuning(**ON):
        on = w.index.search(COUNT, queries=w.queries[:5], search_k=SK, oversampling=1, raw=True, filters=[f])
    same(on, off)
    live1, _ = _lib.device_cache_stats(w.ds.device)
    b1 = f.info()["device_bytes"]
    assert b1 - b0 >= 125 * 4 and live1 - live0 == b1 - b0, (b0, b1, live0, live1)
    xs = w.index.exhausted_stats()
    assert xs["lists_made"] == 1 and xs["list_ids"] == 125 and xs["leaves_walked"] >= 1, xs
    f.close()
    assert _lib.device_cache_stats(w.ds.device)[0] == live0 - b0
