"""One query on several blocks (k_descend_multi, search.hip): every way its trees can be dealt.

Tree t of a query goes to block g, octet o by t = g + G o (stride 8 G), with G = min(16, ceil(trees / AH_SEARCH_MULTI_TREES_PER_BLOCK))
blocks per query.  The other modules run 9, 12 and 44 trees at 8 trees per block (G = 2, 2, 6).  Here one 200-tree forest gives
indexes over its first T = 16, 100, 128, 129 and 200 trees, searched with 8, 1, 3 and 5 trees per block:

* G = 2 ... 16, the cap of 16 blocks reached from either side (T = 16 at one tree per block, T = 200 at eight);
* blocks with idle octets (T = 16: one tree per block, or three: six blocks of which some hold two trees) and octets that start
  with two roots in their queue (T = 129: one such octet, T = 200: 72 of the 128);
* more than 128 trees, where the 128 lists of a query's control block are all in use and share the exchange wave's two per lane;
* 1, 3 and 32 queries a call (32 x 16 blocks is the largest grid), half of the queries exact copies of stored rows;
* the hand-over at AH_SEARCH_MULTI_MAX_QUERIES, and calls with different block counts one after the other on one index (the last
  block of a query wipes the control block; a stale word of a wider call would show in the next one).

Ids and distance bits must equal the oracle's `nns_by_leaf` (src/reader.rs:317-401) over the same trees, which are the oracle's
own node for node.  Continuous random rows: two trees never hold equal keys at the cut, so no query is handed back for that.

The host gate (ah_search_batch: `block_fits`, an estimate of the leaves a query opens per octet of a descent wave) is restated
here.  At search_k = 1000 it lets every call of this module through.  test_gated_call_* asks for search_k = 8000 on the 16-tree
index — an estimate of more than 8 leaves per octet: the call starts on the wave descent (descent_multi == 0); with
AH_SEARCH_SMALL_GATE=0 it starts on k_descend_multi whatever the estimate says.  Measured on an MI355X: see the test's docstring."""
import numpy as np
import pytest

from arroy_amd import _lib
from arroy_amd import distances as D
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N, DIMS, SPLIT_AFTER, TREES = 6000, 32, 100, 200
T_VALUES = [16, 100, 128, 129, 200]
PER_BLOCK = [8, 1, 3, 5]
NQ = [1, 3, 32]
COUNT, SEARCH_K = 10, 1000  # ~15 leaves of 50 - 100 ids a query: about one per octet list at T = 16, far below the 32 a list holds
MAX_BLOCKS, MAX_QUERIES, SMALL_VISITS = 16, 32, 2048  # kMultiMaxBlocks, kMultiMaxQueries, kSmallVisits (search.hip)


def blocks_per_query(trees, per_block):
    """`multi_blocks` of launch_wave (search.hip)."""
    per_block = min(8, max(1, per_block))
    return min(MAX_BLOCKS, (trees + per_block - 1) // per_block)


def block_fits(forest, trees, search_k):
    """The host's gate on the block descents (ah_search_batch): at most 8 estimated leaves per octet."""
    leaves = forest.nodes["kind"] == 1
    mean_leaf = max(1.0, float(forest.nodes["count"][leaves].sum()) / int(leaves.sum()))
    est_leaves = 1.25 * search_k / mean_leaf + 2.0
    return est_leaves / max(1, min(trees, 32)) <= 8.0


@pytest.fixture(scope="module")
def world():
    import arroy_amd
    from arroy_amd import Dataset
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    rng = np.random.default_rng(2024)
    vecs = rng.standard_normal((N, DIMS)).astype(np.float32)
    ds = Dataset(D.Euclidean, DIMS, N)
    ds.upload_vectors(np.arange(N, dtype=np.uint32), vecs)
    ds.finalize()
    od = O.Data(O.EUCLIDEAN, vecs)
    seeds = [int(x) for x in np.random.default_rng(7).integers(0, 2**63, TREES)]
    ref = [od.build_tree(SPLIT_AFTER, s).canonical() for s in seeds]
    queries = rng.standard_normal((32, DIMS)).astype(np.float32)
    queries[0::2] = vecs[rng.choice(N, 16, replace=False)]  # half of them exact copies of rows
    leaves = [od.query_leaf(q) for q in queries]
    per_t = {}
    for T in T_VALUES:
        forest = ds.build_forest(seeds[:T], split_after=SPLIT_AFTER)
        for t in range(T):
            assert forest.canonical(t) == ref[t], f"tree {t} of the {T}-tree forest differs from the oracle"
        per_t[T] = (forest, ds.create_index(forest), O.forest_view(forest), {})
    yield od, queries, leaves, per_t
    _lib.check(_lib.lib().ah_tuning_reset())
    for forest, index, _view, _want in per_t.values():
        index.close()
        forest.close()
    ds.close()


def oracle_answers(world, T, nq, search_k=SEARCH_K):
    """The oracle's (ids, distances) of the first nq queries over the first T trees; computed once per (T, search_k)."""
    od, _queries, leaves, per_t = world
    forest, _index, view, cache = per_t[T]
    for qi in range(nq):
        if (qi, search_k) not in cache:
            want, _ = O.search(od, forest, *leaves[qi], COUNT, search_k, want_candidates=False, view=view)
            cache[qi, search_k] = ([i for i, _ in want], np.array([d for _, d in want], dtype=np.float32))
    return [cache[qi, search_k] for qi in range(nq)]


def assert_equals_oracle(got, want, what):
    oi, od_, oc = got
    for qi, (ids, dist) in enumerate(want):
        assert int(oc[qi]) == len(ids) and list(oi[qi, : oc[qi]]) == ids, f"{what}: ids of query {qi}"
        assert od_[qi, : oc[qi]].tobytes() == dist.tobytes(), f"{what}: distances of query {qi}"


@pytest.mark.parametrize("per_block", PER_BLOCK)
@pytest.mark.parametrize("T", T_VALUES)
def test_every_deal_of_trees_over_blocks_equals_the_oracle(world, T, per_block):
    _od, queries, _leaves, per_t = world
    forest, index, _view, _ = per_t[T]
    G = blocks_per_query(T, per_block)
    assert G == {(16, 8): 2, (16, 1): 16, (16, 3): 6, (16, 5): 4, (100, 8): 13, (100, 5): 16, (128, 8): 16, (129, 8): 16,
                 (200, 8): 16}.get((T, per_block), 16)
    assert block_fits(forest, T, SEARCH_K)  # the host gate lets every call of this test start on the block descents
    for nq in NQ:
        what = f"T = {T}, {per_block} trees per block (G = {G}), nq = {nq}"
        with _lib.tuning(AH_SEARCH_MULTI_TREES_PER_BLOCK=per_block):
            index.stats(reset=True)
            got = index.search(COUNT, queries=queries[:nq], search_k=SEARCH_K, raw=True)
            st = index.stats()
        print(what, {k: v for k, v in st.items() if v})
        assert_equals_oracle(got, oracle_answers(world, T, nq), what)
        # what launch_wave computes: the multi kernel runs iff G >= 2 and nq <= min(AH_SEARCH_MULTI_MAX_QUERIES, 32)
        assert G >= 2 and nq <= min(_lib.tuning_get("AH_SEARCH_MULTI_MAX_QUERIES")[0], MAX_QUERIES)
        assert st["descent_multi"] == nq and st["fallback_chunks"] == 0, (what, st)


def test_max_queries_hands_a_call_over_to_the_block_descent(world):
    _od, queries, _leaves, per_t = world
    for T in (100, 200):
        _forest, index, _view, _ = per_t[T]
        with _lib.tuning(AH_SEARCH_MULTI_MAX_QUERIES=2):
            for nq, multi in ((3, 0), (1, 1), (2, 2)):
                index.stats(reset=True)
                got = index.search(COUNT, queries=queries[:nq], search_k=SEARCH_K, raw=True)
                st = index.stats()
                assert_equals_oracle(got, oracle_answers(world, T, nq), f"T = {T}, AH_SEARCH_MULTI_MAX_QUERIES = 2, nq = {nq}")
                assert st["descent_multi"] == multi and st["descent_block"] == nq and st["fallback_chunks"] == 0, (T, nq, st)


def test_calls_with_different_block_counts_follow_one_another(world):
    """The control block of a context is shared by all calls: G = 16 leaves 128 lists to wipe, the next call (G = 2 ... 13) reads
    the first of them again, then a wider one again.  Three rounds, 1 and 3 queries alternating."""
    _od, queries, _leaves, per_t = world
    for T in (129, 200):
        _forest, index, _view, _ = per_t[T]
        index.stats(reset=True)
        calls = 0
        for rnd in range(3):
            for per_block in (1, 8, 3, 8, 5, 1):
                nq = 1 if (calls & 1) else 3
                with _lib.tuning(AH_SEARCH_MULTI_TREES_PER_BLOCK=per_block):
                    got = index.search(COUNT, queries=queries[:nq], search_k=SEARCH_K, raw=True)
                assert_equals_oracle(got, oracle_answers(world, T, nq), f"T = {T}, round {rnd}, {per_block} trees per block, nq = {nq}")
                calls += 1
        st = index.stats()
        assert st["descent_multi"] == st["queries"] == 9 * 3 + 9 * 1 and st["fallback_chunks"] == 0, (T, st)
    # ... and from one index to the other (the contexts belong to the dataset): 16 trees on 16 blocks after 200 trees on 16
    for T, per_block in ((200, 8), (16, 1), (200, 1), (16, 8)):
        with _lib.tuning(AH_SEARCH_MULTI_TREES_PER_BLOCK=per_block):
            got = per_t[T][1].search(COUNT, queries=queries[:3], search_k=SEARCH_K, raw=True)
        assert_equals_oracle(got, oracle_answers(world, T, 3), f"T = {T}, {per_block} trees per block after another index")


@pytest.mark.parametrize("nq", [1, 32])
def test_gated_call_takes_the_wave_descent_and_the_ungated_one_still_answers_right(world, nq):
    """search_k = 8000 on 16 trees: ~115 leaves a query, an estimate of ~9 per octet — past the gate's 8.  By design the call
    does not start on the block descents.  With the gate off it does: 32 such queries open more leaf visits than k_units_small
    places (2048) and are redone the long way; one query either fits the 32 leaves of each of its lists or is redone as well.
    What happened on an MI355X: the single query ran on k_descend_multi to the end (descent_multi = 1, 121 leaf visits, no
    chunk redone); the 32 queries gave up (fallback_chunks = 1 with fallback_queue = 1 and fallback_visits = 1, descent_multi
    = 0) and were answered by the sorted path.  Both answers equal the oracle's."""
    _od, queries, _leaves, per_t = world
    T, search_k = 16, 8000
    forest, index, _view, _ = per_t[T]
    assert not block_fits(forest, T, search_k)
    want = oracle_answers(world, T, nq, search_k)
    index.stats(reset=True)
    got = index.search(COUNT, queries=queries[:nq], search_k=search_k, raw=True)
    st = index.stats()
    assert_equals_oracle(got, want, f"gated, nq = {nq}")
    assert st["descent_multi"] == 0 and st["descent_block"] == 0 and st["fallback_chunks"] == 0, st
    with _lib.tuning(AH_SEARCH_SMALL_GATE=0):
        index.stats(reset=True)
        got = index.search(COUNT, queries=queries[:nq], search_k=search_k, raw=True)
        st = index.stats()
    print(f"gate off, nq = {nq}:", {k: v for k, v in st.items() if v})
    assert_equals_oracle(got, want, f"gate off, nq = {nq}")
    assert st["descent_multi"] == nq or st["fallback_chunks"] >= 1, st  # it ran to the end, or gave up and was redone
    # the next small call finds the control block clean
    index.stats(reset=True)
    got = index.search(COUNT, queries=queries[:3], search_k=SEARCH_K, raw=True)
    assert_equals_oracle(got, oracle_answers(world, T, 3), "the call after")
    assert index.stats()["descent_multi"] == 3 and index.stats()["fallback_chunks"] == 0
