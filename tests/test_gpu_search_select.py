"""The selections of ah_search_batch (arroy_amd/csrc/search.hip) at their capacity, and every step `search_chunk` degrades
by when one of them gives up: k_search_select (Euclidean; Cosine / DotProduct with the screen off), k_search_select_screened
(binary16 or int8 first) and its fused variant, which de-duplicates in LDS and writes into pinned memory itself.  Each holds
1024 keys; one more raises bit 3 of the status word, an int8 sub-batch then runs once more on the binary16 rows
(`screen8_retried_chunks`, noted in a window of 64 sub-batches: eight notes switch the int8 stage of the index off), and
anything else is redone by the sorted path (`fallback_chunks`, `fallback_select`).

Everything goes through the C ABI.  Every answer — ids, distance bits, counts, padding — is the oracle's `O.search` over the
same forest, and for the cases of chosen distances also numpy's on those distances; every statement about a path is read from
`Index.stats()`, reset before the call.  Inputs: search_select_inputs.py; test_search_select_cpu.py proves without a GPU that
each has the property it is named for.  Nothing here provokes a fault: every degraded case is one the library is specified
to answer by another path.

Calls of 1, 8, 32 and 70 queries pick different kernels (the fused selection where the id bitmap fits LDS; every query's descent
writing its own units; k_units_small; past the small kernels), asserted through `descent_block` and `descent_multi`.  The int8
stage takes calls of more than 8 queries only (AH_SEARCH_SMALL_TILES_MAX_QUERIES), so its cases run at 32 and 70."""
import numpy as np
import pytest

import search_select_inputs as S
from arroy_amd import Dataset, _lib
from arroy_amd import distances as D
from arroy_amd.dataset import Index
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CLS = {"dot": D.DotProduct, "euclid": D.Euclidean, "cosine": D.Cosine}
INT8 = {"AH_SCREEN8": 1, "AH_SEARCH_SCREEN8_MIN_QUERIES": 1, "AH_SEARCH_SCREEN8_MAX_VISITS": 128}  # (one leaf a tree: every query visits it)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class World:
    """Rows on the device and in the oracle, and an index over trees of one list each (search_select_inputs.views)."""

    def __init__(self, cls, vectors, trees, ids=None, int8=False):
        n, dims = vectors.shape
        self.ids = np.arange(n, dtype=np.uint32) if ids is None else ids
        self.ds = Dataset(cls, dims, n)
        self.ds.upload_vectors(self.ids, vectors)
        self.oracle = O.Data(cls.metric, vectors, ids=ids)
        if cls.metric == O.DOT_PRODUCT:
            self.ds.preprocess_dot()
            self.oracle.preprocess_dot()
        self.ds.finalize()
        self.view, self.oview, self._keep, self.listed = S.views(trees, cls.metric, dims)
        self.n_trees, self.int8 = len(trees), int8
        self.index = self.new_index()

    def new_index(self):
        if self.int8:  # (the int8 copy of the rows is made with the index: kept whatever its quality figure says)
            with _lib.tuning(AH_SCREEN8=1):
                return Index(self.ds, None, view=self.view)
        return Index(self.ds, None, view=self.view)

    def search(self, count, queries, cand=None, **tun):
        """-> (ids, distances, counts), the stats of this call"""
        with _lib.tuning(**tun):
            self.index.stats(reset=True)
            got = self.index.search(count, queries=queries, search_k=self.listed, candidates=cand, candidates_sorted=True, raw=True)
            return got, self.index.stats()

    def want(self, q, count, cand=None):
        qv, qh = self.oracle.query_leaf(q)
        res, _ = O.search(self.oracle, None, qv, qh, count, self.listed, 0, cand, candidates_sorted=True, want_candidates=False,
                          view=self.oview)
        return np.array([i for i, _ in res], dtype=np.uint32), np.array([d for _, d in res], dtype=np.float32)

    def check(self, got, queries, count, picks, cand=None, what=None):
        oi, od, oc = got
        for qi in picks:
            wi, wd = self.want(queries[qi], count, cand)
            m = len(wi)
            assert int(oc[qi]) == m and oi[qi, :m].tolist() == wi.tolist(), (what, qi)
            assert bits(od[qi, :m]).tolist() == bits(wd).tolist(), (what, qi)
            assert np.all(oi[qi, m:] == 0xFFFFFFFF) and np.all(bits(od[qi, m:]) == 0xFFFFFFFF), (what, qi)

    def close(self):
        self.index.close()
        self.ds.close()


def nz(st):
    return {f: v for f, v in st.items() if v}


def shape_of(st, nq, n_trees):
    """Which descent took a served, unfiltered call of nq queries: a block per query up to 64 queries a call, the trees of a
    query dealt over several blocks (nine trees and more) up to 32."""
    assert st["descent_block"] == (nq if nq <= 64 else 0), (nq, nz(st))
    assert st["descent_multi"] == (nq if nq <= 32 and n_trees >= 9 else 0), (nq, nz(st))
    assert st["queries"] == nq and st["chunks"] == 1 and st["rerank_tiles"] == nq and st["rerank_sorted"] == 0, (nq, nz(st))


def served(st, nq):
    assert st["rerank_tiles"] == nq and st["fallback_chunks"] == 0 and st["rerank_sorted"] == 0, (nq, nz(st))
    assert st["fallback_select"] == st["fallback_non_finite"] == st["fallback_queue"] == st["fallback_visits"] == st["fallback_launch"] == 0, nz(st)


def left_to_the_sorted_path(st, nq, reason="fallback_select"):
    assert st["fallback_chunks"] == 1 and st[reason] == 1 and st["rerank_sorted"] == nq and st["rerank_tiles"] == 0, (nq, reason, nz(st))
    for other in ("fallback_select", "fallback_non_finite", "fallback_queue", "fallback_visits", "fallback_launch"):
        assert other == reason or st[other] == 0, (nq, reason, nz(st))


# ---- a. the unscreened selection at its capacity -------------------------------------------------------------------------------

CASES = S.capacity_cases()


@pytest.mark.parametrize("sparse", [False, True], ids=["identity-ids", "sparse-ids"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_unscreened_selection_at_its_capacity(case, sparse):
    """k_search_select: 1024 selected keys are served by the tiles, 1025 are left to the sorted path — by equal distances
    around the k-th place and by distinct distances in the k-th key's bin, over direct and scaled spans, with the k-th key on
    the first and on the last word of its bin, fewer distinct candidates than count, a filter that keeps nothing and one that
    keeps exactly count, and the same ids in every tree.  DotProduct with the screen on: the same answers, whatever serves."""
    ids = case.ids(sparse)
    w = World(CLS[case.metric], case.vectors, case.trees(sparse), ids=ids if sparse else None)
    cand = None if case.keep is None else ids[case.keep]
    try:
        for nq in S.SHAPES:
            qs = case.queries(nq)
            got, st = w.search(case.count, qs, cand, AH_SEARCH_SCREEN=0)
            assert st["rerank_screened"] == 0 and st[("dedup_flag_hash" if sparse else "dedup_flag_bitmap")] == (nq if case.served else 0), st
            if case.served:
                served(st, nq)
                if cand is None:
                    shape_of(st, nq, w.n_trees)
            else:
                left_to_the_sorted_path(st, nq)
            w.check(got, qs, case.count, (0, nq - 1), cand, (case.name, nq))
            for qi in range(nq):  # ... and numpy's on the chosen distances, every query
                wi, wd = case.expect(qs[qi], sparse)
                assert got[0][qi, :len(wi)].tolist() == wi.tolist() and bits(got[1][qi, :len(wi)]).tolist() == bits(wd).tolist()
                assert int(got[2][qi]) == len(wi)
            if case.metric == "dot" and nq in (1, 70):
                again, _ = w.search(case.count, qs, cand)
                for a, b in zip(got, again):
                    assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b), (case.name, nq)
    finally:
        w.close()


# ---- b. the screened selections at their capacity ---------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True], ids=["identity-ids", "sparse-ids"])
@pytest.mark.parametrize("m", [1024, 1025])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_screened_selections_at_their_capacity(metric, m, sparse):
    """Group A of m copies of one vector: equal bounds, so all of it survives or none.  m = 1024 is served, by the fused
    variant too (identity ids, up to 64 queries a call), and `screen_survivors` says that nothing else survived; m = 1025 is
    left to the sorted path — after the binary16 retry when the int8 rows went first."""
    vecs, a, v = S.screened_case(m)
    n = len(vecs)
    ids = S.sparse_ids(n) if sparse else np.arange(n, dtype=np.uint32)
    w = World(CLS[metric], vecs, S.spread(ids), ids=ids if sparse else None, int8=True)
    count = 1024
    try:
        for nq in S.SHAPES:
            qs = S.screened_queries(v, nq)
            for tun in ({"AH_SEARCH_SCREEN8": 0},) + ((INT8,) if nq > 8 else ()):
                got, st = w.search(count, qs, None, **tun)
                int8 = tun is INT8
                if m == 1024:
                    served(st, nq)
                    shape_of(st, nq, w.n_trees)
                    assert st["rerank_screened"] == nq and st["screen_survivors"] == nq * 1024, (nq, tun, st)
                    assert st["rerank_screened8"] == (nq if int8 else 0) and st["screen8_retried_chunks"] == 0, (nq, tun, st)
                else:
                    left_to_the_sorted_path(st, nq)
                    assert st["screen8_retried_chunks"] == (1 if int8 else 0) and st["rerank_screened"] == 0, (nq, tun, st)
                w.check(got, qs, count, (0, nq - 1), None, (metric, m, nq, tun))
                assert got[0][0].tolist() == ids[a[:1024]].tolist()  # ties broken by id
                if nq <= 64 and not sparse and not int8:
                    # the same call with the de-duplication in a launch of its own: the non-fused selection at the same ids
                    # and shape, the same bits and the same stats (no stat says which of the two ran)
                    plain, st2 = w.search(count, qs, None, AH_SEARCH_FUSED_FLAG=0, **tun)
                    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, plain)), (metric, m, nq)
                    assert {f: st2[f] for f in ("rerank_screened", "screen_survivors", "fallback_select", "rerank_tiles")} == \
                        {f: st[f] for f in ("rerank_screened", "screen_survivors", "fallback_select", "rerank_tiles")}, (nq, nz(st2))
    finally:
        w.close()


# ---- c. the middle of the chain: int8, binary16, sorted -----------------------------------------------------------------------------

def cluster_world(cls, spread_, seed=17):
    """test_gpu_query_screens.clustered: 3000 rows around a centre within `spread_`, 1000 unrelated rows; three trees.
    (DotProduct lists only the members, as there: distances of both signs put the whole cluster into one bin.)"""
    rng = np.random.default_rng(seed)
    vecs, centre = S.clustered(rng, 1000, 3000, 256, spread_)
    listed = np.arange(4000 if cls is D.Cosine else 3000, dtype=np.uint32)
    return World(cls, vecs, S.spread(listed, 3, 2), int8=True), centre


SPREADS = {D.Cosine: (0.15, 0.01), D.DotProduct: (0.03, 0.001)}


@pytest.mark.parametrize("cls", [D.Cosine, D.DotProduct], ids=["cosine", "dot"])
def test_near_ties_retry_on_binary16_then_the_sorted_path(cls):
    """A loose cluster around the query: the int8 stage overflows and binary16 answers; a tight one: binary16 overflows as
    well and the sorted path answers.  Under AH_SCREEN_VERIFY=1 every candidate's reference distance lies in its bounds."""
    k = 10
    for spread_, tight in zip(SPREADS[cls], (False, True)):
        w, centre = cluster_world(cls, spread_)
        try:
            for nq in S.SHAPES:
                qs = np.repeat(centre[None, :], nq, axis=0)
                w.ds.query_screen_verify(reset=True)
                got, st = w.search(k, qs, None, AH_SCREEN_VERIFY=1, **INT8)
                v = w.ds.query_screen_verify()
                print("near ties", cls.__name__, spread_, nq, {f: st[f] for f in ("rerank_screened", "rerank_screened8", "screen8_retried_chunks",
                                                                                  "fallback_chunks", "fallback_select", "screen_survivors")}, v)
                assert v["violations"] == 0 and v["checked"] > 0, v
                assert st["screen8_retried_chunks"] == (1 if nq > 8 else 0) and st["rerank_screened8"] == 0, (nq, st)
                if tight:
                    left_to_the_sorted_path(st, nq)
                    assert st["rerank_screened"] == 0, (nq, st)
                else:
                    served(st, nq)
                    assert st["rerank_screened"] == nq, (nq, st)
                w.check(got, qs, k, (0, nq - 1), None, (cls.__name__, spread_, nq))
        finally:
            w.close()


def test_the_int8_retry_under_the_default_tunables():
    """No tunable set: 70 clusters of 1500 near ties under a built forest, one query at every centre.  A call of 70 queries
    takes the int8 rows first, every query reaches leaves of its own cluster (which no other query visits), all 1500 members
    are within the int8 bound of each other, and the sub-batch is answered by the binary16 retry."""
    from arroy_amd import shard
    rng = np.random.default_rng(71)
    n_clusters, members, dims, k, sk = 70, 1500, 256, 10, 3000
    centres = rng.standard_normal((n_clusters, dims)).astype(np.float32)
    vecs = (np.repeat(centres, members, axis=0) + 0.15 * rng.standard_normal((n_clusters * members, dims))).astype(np.float32)
    n = len(vecs)
    ds = Dataset(D.Cosine, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    ds.finalize()
    forest = ds.build_forest(shard.tree_seeds(71, range(4)))
    index = ds.create_index(forest)
    od = O.Data(O.COSINE, vecs)
    try:
        index.stats(reset=True)
        got = index.search(k, queries=centres, search_k=sk, raw=True)
        st = index.stats()
        assert st["screen8_retried_chunks"] == 1 and st["fallback_chunks"] == 0 and st["rerank_tiles"] == n_clusters, nz(st)
        assert st["rerank_screened"] == n_clusters and st["rerank_screened8"] == 0, nz(st)
        with _lib.tuning(AH_SEARCH_SCREEN8=0, AH_SCREEN_VERIFY=1):
            ds.query_screen_verify(reset=True)
            index.stats(reset=True)
            plain = index.search(k, queries=centres, search_k=sk, raw=True)
            st, v = index.stats(), ds.query_screen_verify()
        assert st["screen8_retried_chunks"] == 0 and st["rerank_screened"] == n_clusters and v["violations"] == 0 and v["checked"] > 0, (nz(st), v)
        for a, b in zip(got, plain):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for qi in (0, 35, 69):
            qv, qh = od.query_leaf(centres[qi])
            want, _ = O.search(od, forest, qv, qh, k, sk, want_candidates=False)
            assert int(got[2][qi]) == len(want) and got[0][qi].tolist() == [i for i, _ in want], qi
            assert bits(got[1][qi]).tolist() == bits(np.array([d for _, d in want], np.float32)).tolist(), qi
    finally:
        index.close()
        forest.close()
        ds.close()


# ---- d. the window of the int8 switch --------------------------------------------------------------------------------------------------

def test_int8_switch_of_an_index_counts_overflows_in_windows_of_64():
    """test_int8_switch_counts_overflows_in_windows_of_64 on an index: eight overflowing sub-batches each followed by 15 good
    ones leave the int8 stage on; eight within one window switch it off for the life of the index — `rerank_screened8` stops,
    `rerank_screened` goes on, the answers stay the oracle's — and a fresh index of the same dataset starts with it on."""
    w, centre = cluster_world(D.Cosine, 0.15, seed=41)
    rng = np.random.default_rng(43)
    nq, k = 32, 10
    near = np.repeat(centre[None, :], nq, axis=0)
    good = (-centre[None, :] + 0.5 * rng.standard_normal((nq, 256))).astype(np.float32)  # (the cluster is the farthest there)
    try:
        with _lib.tuning(**INT8):
            def call(qs):
                return w.index.search(k, queries=qs, search_k=w.listed, raw=True)
            w.index.stats(reset=True)
            for _ in range(8):
                first = call(near)
                for _ in range(15):
                    call(good)
            st = w.index.stats()
            assert st["screen8_retried_chunks"] == 8 and st["rerank_screened8"] == 8 * 15 * nq and st["fallback_chunks"] == 0, st
            got = call(good)
            assert w.index.stats()["rerank_screened8"] == (8 * 15 + 1) * nq
            w.check(got, good, k, (0, nq - 1))
            w.check(first, near, k, (0,))
            # eight within 64: switched off
            w.index.close()
            w.index = w.new_index()
            w.index.stats(reset=True)
            for _ in range(8):
                call(near)
                call(good)
            st = w.index.stats()
            assert st["screen8_retried_chunks"] == 8 and st["rerank_screened8"] == 7 * nq, st  # the 8th overflow switched it off
            assert st["rerank_screened"] == 16 * nq and st["fallback_chunks"] == 0, st
            got = call(good)
            near_off = call(near)
            st = w.index.stats()
            assert st["rerank_screened8"] == 7 * nq and st["screen8_retried_chunks"] == 8 and st["rerank_screened"] == 18 * nq, st
            w.check(got, good, k, (0, nq - 1))
            w.check(near_off, near, k, (0, nq - 1))
            # a fresh index on the same dataset starts with the stage on
            w.index.close()
            w.index = w.new_index()
            w.index.stats(reset=True)
            call(good)
            assert w.index.stats()["rerank_screened8"] == nq
    finally:
        w.close()


# ---- e. a good call after a degraded one ---------------------------------------------------------------------------------------------------

def alternate(w, count, nq, degraded, ordinary, reason, tun_degraded=None, tun=None, retried=0, what=None, cand=None):
    """Three times a degraded call and an ordinary one, on this thread's context: each degraded call counts its reason once,
    each ordinary one is served with nothing redone, and both give the oracle's bits.  `cand`: a filter of the ordinary calls."""
    for rep in range(3):
        got, st = w.search(count, degraded, None, **(tun_degraded or tun or {}))
        if reason is None:
            served(st, nq)
        else:
            left_to_the_sorted_path(st, nq, reason)
        assert st["screen8_retried_chunks"] == retried, (what, rep, st)
        w.check(got, degraded, count, (0, nq - 1), None, (what, rep, "degraded"))
        got, st = w.search(count, ordinary, cand, **(tun or {}))
        served(st, nq)
        assert st["screen8_retried_chunks"] == 0, (what, rep, st)
        w.check(got, ordinary, count, (0, nq - 1), cand, (what, rep, "ordinary"))


@pytest.mark.parametrize("nq", S.SHAPES)
def test_a_good_call_after_a_degraded_one(nq):
    """The failure paths leave the status block, the pinned status word (preset to 0xFFFFFFFF and polled by the fused path of
    a small call) and the context's memory of a wiped block in another state than a success does.  Same index, same count,
    same number of queries, hence the same scratch layout: the queries alone decide."""
    # fallback_select behind the screened selections: 1025 copies are the nearest of v, and the farthest of -v; and
    # fallback_non_finite there: a query long enough for every dot product to overflow (one sign a row: no NaN)
    vecs, a, v = S.screened_case(1025)
    w = World(D.DotProduct, vecs, S.spread(np.arange(len(vecs), dtype=np.uint32)), int8=True)
    try:
        towards, away = S.screened_queries(v, nq), S.screened_queries(-v, nq, seed=7)
        alternate(w, 10, nq, towards, away, "fallback_select", tun={"AH_SEARCH_SCREEN8": 0}, what="screened")
        alternate(w, 10, nq, towards * np.float32(3e37), away, "fallback_non_finite", tun={"AH_SEARCH_SCREEN8": 0}, what="non-finite, screened")
        if nq > 8:  # int8 first: the retry on binary16, then the sorted path
            alternate(w, 10, nq, towards, away, "fallback_select", tun=INT8, retried=1, what="int8 first")
    finally:
        w.close()
    # fallback_select and fallback_non_finite behind k_search_select: DotProduct with the screen off
    case = next(c for c in CASES if c.name == "ties-direct-1025")
    w = World(D.DotProduct, case.vectors, case.trees(False))
    try:
        qs = case.queries(nq)
        back = qs * np.float32([-1] + [1] * (S.DIMS - 1))  # the same rows seen from the other side: the 600 farthest are distinct
        alternate(w, case.count, nq, qs, back, "fallback_select", tun={"AH_SEARCH_SCREEN": 0}, what="unscreened")
        huge = qs.copy()
        huge[:, 0] = np.finfo(np.float32).max  # -(s * c) overflows for every |c| > 1
        alternate(w, case.count, nq, huge, back, "fallback_non_finite", tun={"AH_SEARCH_SCREEN": 0}, what="non-finite, unscreened")
    finally:
        w.close()
    # Euclidean rows scaled by 3e19 (the squares overflow), as test_device_search_leaf_tiles_leave_non_finite_distances_...;
    # the ordinary call is the same one under a filter that leaves those rows out (the rest fits the selection all the more)
    case = next(c for c in CASES if c.name == "euclid-ties-1024")
    vectors = case.vectors.copy()
    vectors[case.listed[::7]] *= np.float32(3e19)
    finite = np.setdiff1d(np.arange(len(vectors)), case.listed[::7]).astype(np.uint32)
    w = World(D.Euclidean, vectors, case.trees(False))
    try:
        qs = case.queries(nq)
        assert S.selection(S.ordered_words(case.distances(qs[0])[np.setdiff1d(case.listed, case.listed[::7])]), case.count)["served"]
        alternate(w, case.count, nq, qs, qs, "fallback_non_finite", what="rows scaled by 3e19", cand=finite)
    finally:
        w.close()
    # the int8 retry that binary16 answers (no sorted path): the loose cluster
    if nq > 8:
        w, centre = cluster_world(D.Cosine, 0.15)
        rng = np.random.default_rng(nq)
        try:
            near = np.repeat(centre[None, :], nq, axis=0)
            good = (-centre[None, :] + 0.5 * rng.standard_normal((nq, 256))).astype(np.float32)
            alternate(w, 10, nq, near, good, None, tun=INT8, retried=1, what="int8 retry")
        finally:
            w.close()


@pytest.fixture(scope="module")
def built():
    """40 000 x 64 rows under 44 built trees with leaves of at most 64 ids (test_gpu_small_calls.py)."""
    from arroy_amd import shard
    n, dims, trees = 40_000, 64, 44
    vecs = O.synth(11, 2, n, dims)
    ds = Dataset(D.Cosine, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    ds.finalize()
    od = O.Data(O.COSINE, vecs)
    forest = ds.build_forest(shard.tree_seeds(11, range(trees)))
    index = ds.create_index(forest)
    yield ds, od, forest, index, vecs
    index.close()
    forest.close()
    ds.close()


@pytest.mark.parametrize("nq", S.SHAPES)
def test_a_good_call_after_a_queue_overflow(built, nq):
    """`fallback_queue` as test_one_query_on_several_compute_units_... provokes it: a search_k that makes a queue pop more
    leaves than the descent of the call's shape holds, with the host's estimate switched off — k_descend_multi up to 32
    queries, k_descend_block up to 64, both with nothing behind them on the tile path, and the LDS queue of k_descend beyond.
    Each raises bit 4 of the status word; `fallback_visits` (bit 5: more visits than the tile path places) may come with it."""
    _ds, od, forest, index, vecs = built
    rng = np.random.default_rng(5 + nq)
    n = len(vecs)
    qs = (vecs[rng.choice(n, nq, replace=False)] + rng.standard_normal((nq, vecs.shape[1])).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    count = 20
    # (past 64 queries the queue is k_descend's: 1024 entries in LDS, which the frontier of a few hundred leaves does not fill)
    sk_big = n // 2 if nq <= 64 else 4 * n

    def check(got, sk):
        for qi in (0, nq - 1):
            qv, qh = od.query_leaf(qs[qi])
            want, _ = O.search(od, forest, qv, qh, count, sk, want_candidates=False)
            assert got[0][qi, :got[2][qi]].tolist() == [i for i, _ in want], (sk, qi)
            assert bits(got[1][qi, :len(want)]).tolist() == bits(np.array([d for _, d in want], np.float32)).tolist(), (sk, qi)
    for rep in range(3):
        with _lib.tuning(AH_SEARCH_SMALL_GATE=0):
            index.stats(reset=True)
            big = index.search(count, queries=qs, search_k=sk_big, raw=True)
            st = index.stats()
        print("queue overflow", nq, rep, nz(st))
        assert st["fallback_chunks"] == 1 and st["fallback_queue"] == 1 and st["fallback_visits"] <= 1, (rep, nz(st))
        assert st["descent_multi"] == 0 and st["rerank_sorted"] == nq and st["rerank_tiles"] == 0, (rep, nz(st))
        assert st["fallback_select"] == st["fallback_non_finite"] == st["fallback_launch"] == 0, (rep, nz(st))
        check(big, sk_big)
        index.stats(reset=True)
        got = index.search(count, queries=qs, search_k=2000, raw=True)
        st = index.stats()
        assert st["fallback_chunks"] == 0 and st["rerank_tiles"] == nq and st["rerank_sorted"] == 0, (rep, nz(st))
        assert st["descent_multi"] == (nq if nq <= 32 else 0) and st["descent_block"] == (nq if nq <= 64 else 0), (rep, nz(st))
        check(got, 2000)


# ---- f. two sub-batches ----------------------------------------------------------------------------------------------------------------------

def test_the_last_sub_batch_of_a_call_overflows_alone():
    """4100 queries are cut at 4096; of the four queries of the second sub-batch the last one's candidates overflow the
    selection (the same rows, seen from the other side by every other query), so that sub-batch alone is redone."""
    case = next(c for c in CASES if c.name == "ties-direct-1025")
    w = World(D.DotProduct, case.vectors, case.trees(False, 3, 2))
    try:
        qs = case.queries(4100)
        qs[:4099, 0] *= -1
        assert S.selection(case.words(qs[4099]), case.count)["n_sel"] == 1025
        for qi in (0, 1, 2, 3, 4095, 4096, 4097, 4098):
            assert S.selection(case.words(qs[qi]), case.count)["n_sel"] == case.count
        got, st = w.search(case.count, qs, None, AH_SEARCH_SCREEN=0)
        assert st["chunks"] == 2 and st["queries"] == 4100 and st["fallback_chunks"] == 1 and st["fallback_select"] == 1, st
        assert st["rerank_tiles"] == 4096 and st["rerank_sorted"] == 4, st
        w.check(got, qs, case.count, (0, 1, 2, 3, 1000, 2047, 4094, 4095, 4096, 4097, 4098, 4099))
        for qi in range(0, 4100, 41):
            wi, wd = case.expect(qs[qi], False)
            assert got[0][qi].tolist() == wi.tolist() and bits(got[1][qi]).tolist() == bits(wd).tolist(), qi
    finally:
        w.close()


# ---- g. count from 1025 to 2048 ----------------------------------------------------------------------------------------------------------------

def test_counts_beyond_the_capacity_go_straight_to_the_sorted_path():
    """2200 distinct candidates.  count = 1024 is served by the selection; 1025, 1500 and 2048 can only overflow it (it
    holds 1024 keys and selects at least min(count, distinct candidates)), so such a call starts on the sorted path: no tile
    pass, nothing redone.  (Measured while the tiles were gated on count <= 2048 only: every such sub-batch, at every call
    shape, did the whole tile pass, raised bit 3 and was redone — `fallback_select` — after an int8 pass and a binary16 retry
    where the int8 stage was on.)"""
    case = S.big_count_case()
    w = World(D.DotProduct, case.vectors, case.trees(False))
    try:
        for nq in S.SHAPES:
            qs = case.queries(nq)
            for count in S.BIG_COUNTS:
                for tun in ({"AH_SEARCH_SCREEN": 0}, {}):
                    got, st = w.search(count, qs, None, **tun)
                    print("count", count, "queries", nq, tun, {f: st[f] for f in ("rerank_tiles", "rerank_sorted", "fallback_chunks",
                                                                                 "fallback_select", "rerank_screened")})
                    if count <= S.CAP:
                        if tun:  # (the screen cannot tell distances apart that differ in their last bits: either path may serve)
                            served(st, nq)
                    else:
                        assert st["rerank_sorted"] == nq and st["rerank_tiles"] == 0 and st["fallback_chunks"] == 0, (count, nq, st)
                    w.check(got, qs, count, (0, nq - 1), None, (count, nq))
                    wi, wd = case.expect(qs[nq - 1], False, count)
                    assert got[0][nq - 1].tolist() == wi.tolist() and bits(got[1][nq - 1]).tolist() == bits(wd).tolist()
    finally:
        w.close()


def test_counts_beyond_the_capacity_over_a_candidate_buffer_within_it_stay_on_the_tiles():
    """count = 1500 meant as "everything": one tree of 700 ids, so a query's candidate buffer cannot hold more than the
    selection does and the tiles serve the call as they did before counts were gated."""
    case = next(c for c in CASES if c.name == "unique-below-count")
    w = World(D.DotProduct, case.vectors, case.trees(False, 1))
    assert w.listed == 700 <= S.CAP
    try:
        for nq in S.SHAPES:
            qs = case.queries(nq)
            for tun in ({"AH_SEARCH_SCREEN": 0}, {"AH_SEARCH_TILES": 0}):
                got, st = w.search(1500, qs, None, **tun)
                if "AH_SEARCH_TILES" in tun:
                    assert st["rerank_sorted"] == nq and st["fallback_chunks"] == 0, nz(st)
                else:
                    served(st, nq)
                assert got[2].tolist() == [700] * nq
                w.check(got, qs, 1500, (0, nq - 1), None, (nq, tun))
                wi, wd = case.expect(qs[nq - 1], False, 1500)
                assert got[0][nq - 1, :700].tolist() == wi.tolist() and bits(got[1][nq - 1, :700]).tolist() == bits(wd).tolist()
    finally:
        w.close()


def test_counts_beyond_the_capacity_leave_the_int8_stage_on():
    """Eight calls of count = 1500 (70 queries, int8 first) used to note eight int8 failures within one window and switch
    the stage off for every later search of the index, whatever its count."""
    vecs, a, v = S.screened_case(1024)
    w = World(D.Cosine, vecs, S.spread(np.arange(len(vecs), dtype=np.uint32)), int8=True)
    nq = 70
    qs = S.screened_queries(v, nq)
    try:
        for _ in range(8):
            got, st = w.search(1500, qs, None, **INT8)
            assert st["rerank_sorted"] == nq and st["fallback_chunks"] == 0 and st["screen8_retried_chunks"] == 0, st
        w.check(got, qs, 1500, (0, nq - 1))
        got, st = w.search(10, qs, None, **INT8)
        served(st, nq)
        assert st["rerank_screened8"] == nq and st["screen8_retried_chunks"] == 0, st
        w.check(got, qs, 10, (0, nq - 1))
    finally:
        w.close()
