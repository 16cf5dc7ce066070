"""The leaf tiles of the three 1-bit metrics (AH_SEARCH_TILES_BQ=1; DESIGN.md §4 "1-bit leaf tiles").  Every call runs at 1 and at 0:
equal ids, distance bits and counts, the oracle's for the picked queries, and `Index.stats` says which path ran."""
import functools

import numpy as np
import pytest

from arroy_amd import Dataset, _lib, shard
from arroy_amd import distances as D
from arroy_amd.dataset import Index
from oracle import oracle as O
from test_gpu_parity import _equal_keys_fixture
from test_gpu_query_screens import bits, make, same
from test_gpu_search_diff import LADDER, queries_near

pytestmark = pytest.mark.gpu
METRICS = pytest.mark.parametrize("cls", [D.BinaryQuantizedEuclidean, D.BinaryQuantizedManhattan, D.BinaryQuantizedCosine],
                                  ids=["bq-euclidean", "bq-manhattan", "bq-cosine"])
COUNT, SK = 10, 600


@functools.lru_cache(maxsize=None)
def built(cls, dims, ties=False, n=2000, trees=5):
    """Five trees: 1-bit margins tie so often that a query's queue holds most leaves of every tree, and past 1024 entries the
    sub-batch takes the sorted path (fallback_queue).  ties: row i is all ones with eighth i % 8 of its dimensions negated."""
    X = np.random.default_rng(dims).standard_normal((n, dims)).astype(np.float32)
    if ties:
        X = 1 - 2 * (np.arange(dims) // (dims // 8) == np.arange(n)[:, None] % 8).astype(np.float32)
    ds, oracle = make(cls, X)
    forest = ds.build_forest(shard.tree_seeds(42, range(trees)))
    return ds, oracle, forest, ds.create_index(forest), X


def both(index, oracle, forest, count, sk, picks, tun={}, keep=None, **kw):
    """The same search at 1 and at 0: equal answers, 0 on the sorted path, the picked queries the oracle's.  The stats at 1."""
    out = []
    for on in (1, 0):
        with _lib.tuning(AH_SEARCH_TILES_BQ=on, **tun):
            index.stats(reset=True)
            out.append((index.search(count, search_k=sk, raw=True, candidates=keep, **kw), index.stats()))
    (got, st), (ref, st0) = out
    same(got, ref, "setting 1 vs setting 0")
    assert st0["rerank_tiles"] == 0 and st0["rerank_sorted"] > 0, st0
    for i in picks:
        qv, qh = oracle.item_leaf(int(kw["items"][i])) if "items" in kw else oracle.query_leaf(kw["queries"][i])
        want, _ = O.search(oracle, forest, qv, qh, count, sk, candidates=keep, want_candidates=False)
        assert got[0][i, : got[2][i]].tolist() == [a for a, _ in want], i
        assert bits(got[1][i, : got[2][i]]).tolist() == bits(np.array([b for _, b in want], np.float32)).tolist(), i
    return got, st


# Row widths at 24 queries, by 16-byte pieces and lanes per row: 40 -> 1 word, 24 padding bits, one lane; 72 -> 2 words, one full
# piece; 200 -> 2 pieces, 2 lanes; 300 -> 5 words, 3 pieces on 4 lanes; 800 -> 13 words, 7 pieces on 8 lanes, the last half padding;
# 1100 -> 18 words, 9 pieces: past the 8 one pass of an 8-lane group holds, so two passes.  Then the launch ladder at two widths.
CASES = [(d, 24, {}, 0, 0) for d in (40, 72, 200, 300, 800, 1100)] + [(d,) + c for d in (72, 800) for c in LADDER]


@METRICS
@pytest.mark.parametrize("dims,nq,tun,by_item,filtered", CASES, ids=[f"{c[0]}-nq{c[1]}" + "".join(f"-{k[10:]}0" for k in c[2]) +
                                                                     "-item" * c[3] + "-filter" * c[4] for c in CASES])
def test_tiles_answer_as_the_sorted_path(cls, dims, nq, tun, by_item, filtered):
    ds, oracle, forest, index, X = built(cls, dims)
    rng = np.random.default_rng([dims, nq])
    qs = queries_near(X, nq, rng)
    kw = {"items": rng.choice(len(X), nq, replace=False).astype(np.uint32)} if by_item else {"queries": qs}
    keep = np.arange(0, len(X), 2, dtype=np.uint32) if filtered else None
    st = both(index, oracle, forest, COUNT, SK, {0, nq - 1}, tun, keep, **kw)[1]
    assert st["rerank_tiles"] == nq and st["rerank_sorted"] == 0 and st["fallback_chunks"] == 0, st
    if not by_item and not filtered:  # units of more than 8 visits by their counter; few queries: only the smaller classes
        assert (nq < 40 or st["tile_units_16"] > 0) and (nq > 8 or st["tile_units_16"] == 0 < st["tile_units_8"] + st["tile_units_4"]), st


@METRICS
def test_ties_at_the_cut_take_the_sorted_path(cls, dims=200):
    # query 0, the vector of ones, has all 2000 rows at one distance: more keys up to the cut than the selection holds
    ds, oracle, forest, index, X = built(cls, dims, ties=True)
    qs, fell_back = np.stack([np.ones(dims, np.float32), X[0], X[3]]), 0
    for count in (10, 300):
        st = both(index, oracle, forest, count, 12 * len(X), range(3), queries=qs)[1]
        assert st["rerank_tiles"] + st["rerank_sorted"] == 3 and st["fallback_chunks"] == st["fallback_select"], st
        fell_back += st["fallback_select"]
    assert fell_back > 0


def test_recorded_equal_keys_case():
    g, forest = _equal_keys_fixture()
    ds = Dataset(D.BY_METRIC[int(g["metric"])], g["vecs"].shape[1], len(g["vecs"]))
    ds.upload_vectors(g["ids"], g["vecs"])
    ds.finalize()
    (oi, od, oc), st = both(Index(ds, None, view=O.forest_view(forest)), None, None, int(g["count"]), int(g["sk"]), (), queries=np.stack([g["query"]] * 9))
    assert st["rerank_tiles"] == 9 and st["rerank_sorted"] == 0, st
    for qi in range(9):
        assert oi[qi, : oc[qi]].tolist() == g["want_ids"].tolist() and bits(od[qi, : oc[qi]]).tolist() == bits(g["want_dists"]).tolist()


@METRICS
def test_the_width_gate_and_the_default(cls):
    ds, oracle, forest, index, X = built(cls, 64 * 128 + 1, n=300, trees=2)  # 129 words: kBqTileMaxWords + 1
    st = both(index, oracle, forest, COUNT, 200, (0,), queries=X[:3] * np.float32(0.5))[1]
    assert st["rerank_tiles"] == 0 and st["rerank_sorted"] == 3 and st["fallback_chunks"] == 0, st
    assert _lib.tuning_get("AH_SEARCH_TILES_BQ") == (0, 0)  # unset: a width the tiles take stays on the sorted path
    index, X = built(cls, 72)[3:]
    index.stats(reset=True)
    index.search(COUNT, queries=X[:4], search_k=SK, raw=True)
    assert index.stats()["rerank_tiles"] == 0 and index.stats()["rerank_sorted"] == 4, index.stats()
