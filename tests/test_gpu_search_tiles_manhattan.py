"""Manhattan's exact rows through the leaf tiles (AH_SEARCH_TILES_MANHATTAN=1; DESIGN.md §4 "Manhattan leaf tiles").  Every call
runs at 1 and at 0: equal ids, distance bits and counts, the oracle's for the picked queries, and `Index.stats` says which path
ran.  The reference's sum is sequential; at these widths any re-associated sum differs from it in the last bits."""
import functools

import numpy as np
import pytest

from arroy_amd import _lib, shard
from arroy_amd import distances as D
from oracle import oracle as O
from test_gpu_query_screens import bits, make, same

pytestmark = pytest.mark.gpu
COUNT, SK = 10, 600


@functools.lru_cache(maxsize=None)
def built(dims, diff=0):
    """(ds, oracle, forest, index, rows): 2000 standard-normal rows under 5 trees; diff: the index made under AH_SEARCH_SCREEN_DIFF."""
    X = np.random.default_rng(dims).standard_normal((2000, dims)).astype(np.float32)
    ds, oracle = make(D.Manhattan, X)
    forest = ds.build_forest(shard.tree_seeds(42, range(5)))
    with _lib.tuning(AH_SEARCH_SCREEN_DIFF=diff):
        return ds, oracle, forest, ds.create_index(forest), X


def both(index, oracle, forest, picks, keep=None, **kw):
    """The same search at 1 and at 0: equal answers, 0 on the sorted path, the picked queries the oracle's.  The stats at 1."""
    out = []
    for on in (1, 0):
        with _lib.tuning(AH_SEARCH_TILES_MANHATTAN=on):
            index.stats(reset=True)
            out.append((index.search(COUNT, search_k=SK, raw=True, candidates=keep, **kw), index.stats()))
    (got, st), (ref, st0) = out
    same(got, ref, "setting 1 vs setting 0")
    assert st0["rerank_tiles"] == 0 < st0["rerank_sorted"], st0
    for i in picks:
        qv, qh = oracle.item_leaf(int(kw["items"][i])) if "items" in kw else oracle.query_leaf(kw["queries"][i])
        want, _ = O.search(oracle, forest, qv, qh, COUNT, SK, candidates=keep, want_candidates=False)
        assert got[0][i, : got[2][i]].tolist() == [a for a, _ in want], i
        assert bits(got[1][i, : got[2][i]]).tolist() == bits(np.array([b for _, b in want], np.float32)).tolist(), i
    return st


# Widths: 32 -> one chunk, no tail; 37 -> a tail that is no multiple of 4; 72 -> two chunks and a tail; 200 -> several chunks, one
# slab; 333 -> leaves of up to 333 rows (two slabs of 256, three of 128), the accumulators over ten chunk boundaries.  Queries: 24
# near-duplicates (units of 9 - 16 visits), 3 and 1 (the small descents, units of at most 4).  (dims, nq, by item, filtered)
CASES = [(d, nq, 0, 0) for d in (32, 37, 72, 200, 333) for nq in (24, 3, 1)] + [(d, 24, i, 1 - i) for d in (37, 333) for i in (0, 1)]


@pytest.mark.parametrize("dims,nq,by_item,filtered", CASES, ids=[f"{c[0]}-nq{c[1]}" + "-item" * c[2] + "-filter" * c[3] for c in CASES])
def test_tiles_answer_as_the_sorted_path(dims, nq, by_item, filtered):
    ds, oracle, forest, index, X = built(dims)
    rng = np.random.default_rng([dims, nq])
    qs = (X[100] + rng.standard_normal((nq, dims)) * 1e-3).astype(np.float32)
    kw = {"items": rng.choice(len(X), nq, replace=False).astype(np.uint32)} if by_item else {"queries": qs}
    keep = np.arange(0, len(X), 2, dtype=np.uint32) if filtered else None
    st = both(index, oracle, forest, {0, nq - 1}, keep, **kw)
    assert st["rerank_tiles"] == nq and st["rerank_sorted"] == 0 and st["fallback_chunks"] == 0, st
    if not by_item:  # near-duplicates share every leaf: units of more than 8 visits at 24 queries, of at most 4 at 3 and 1
        assert st["tile_units_16"] > 0 if nq == 24 else st["tile_units_16"] == st["tile_units_8"] == 0 < st["tile_units_4"], st


def test_the_difference_screen_keeps_precedence(dims=72, nq=8):
    ds, oracle, forest, index, X = built(dims, diff=1)
    with _lib.tuning(AH_SEARCH_TILES_MANHATTAN=1, AH_SEARCH_SCREEN_DIFF=1):
        index.search_diff_stats(reset=True)
        got = index.search(COUNT, queries=X[:nq] * np.float32(0.5), search_k=SK, raw=True)
        assert index.search_diff_stats()["queries"] == nq, index.search_diff_stats()
    with _lib.tuning(AH_SEARCH_TILES_MANHATTAN=1):  # ... and without the screen the exact tiles give the same bits
        index.stats(reset=True)
        same(got, index.search(COUNT, queries=X[:nq] * np.float32(0.5), search_k=SK, raw=True), "screened vs exact tiles")
        assert index.stats()["rerank_tiles"] == nq, index.stats()


def test_mixed_filters_keep_the_sorted_path_and_the_default_is_off(dims=72, nq=6):
    ds, oracle, forest, index, X = built(dims)
    ids = np.arange(len(X), dtype=np.uint32)
    filters = [index.make_filter(ids[::2].copy(), sorted=True), index.make_filter(ids[1::2].copy(), sorted=True)]
    with _lib.tuning(AH_SEARCH_TILES_MANHATTAN=1, AH_SEARCH_FILTER_GROUP_MIN=nq + 1):
        index.stats(reset=True)
        index.search(COUNT, queries=X[:nq], search_k=SK, raw=True, filters=filters, filter_of_query=np.resize(np.array([0, 1], np.uint32), nq))
        assert index.stats()["rerank_tiles"] == 0 and index.stats()["rerank_sorted"] == nq, index.stats()
    assert _lib.tuning_get("AH_SEARCH_TILES_MANHATTAN") == (0, 0)
    index.stats(reset=True)
    index.search(COUNT, queries=X[:4], search_k=SK, raw=True)
    assert index.stats()["rerank_tiles"] == 0 and index.stats()["rerank_sorted"] == 4, index.stats()
