"""Long candidate lists on an id space past the LDS bitmap through the leaf tiles (AH_SEARCH_FLAG_SLICED=1; DESIGN.md §4 "Sliced
duplicate flags").  4000 rows under 8 trees at search_k 30 000: a candidate stride of 32 768, past the 24 576 of one hash set;
AH_SEARCH_BITMAP=0 takes the bitmap away (one case has ids up to 2.8 M instead).  Every call runs at 1 and at 0: equal ids,
distance bits and counts, the oracle's for the first and last query, and `Index.stats` says which path ran."""
import functools

import numpy as np
import pytest

from arroy_amd import Dataset, _lib, shard
from arroy_amd import distances as D
from oracle import oracle as O
from test_gpu_query_screens import bits, make, same

pytestmark = pytest.mark.gpu
COUNT = 10


@functools.lru_cache(maxsize=None)
def built(cls=D.Euclidean, n=4000, trees=8, id_step=1):
    X = np.random.default_rng(n).standard_normal((n, 32)).astype(np.float32)
    if id_step == 1:
        ds, oracle = make(cls, X)
    else:  # sparse item ids: `make` numbers them 0 .. n - 1
        ids = np.arange(n, dtype=np.uint32) * np.uint32(id_step)
        ds, oracle = Dataset(cls, 32, n), O.Data(cls.metric, X, ids=ids)
        ds.upload_vectors(ids, X)
        ds.finalize()
    forest = ds.build_forest(shard.tree_seeds(42, range(trees)))
    return oracle, forest, ds.create_index(forest), X


def both(oracle, forest, index, sk, keep, tun, **kw):
    """The same search at 1 and at 0: equal answers, the first and last query the oracle's.  The stats at 1 and at 0."""
    out = []
    for on in (1, 0):
        with _lib.tuning(AH_SEARCH_FLAG_SLICED=on, **tun):
            index.stats(reset=True)
            out.append((index.search(COUNT, search_k=sk, raw=True, candidates=keep, **kw), index.stats()))
    (got, st), (ref, st0) = out
    same(got, ref, "setting 1 vs setting 0")
    for i in {0, len(got[2]) - 1}:
        qv, qh = oracle.item_leaf(int(kw["items"][i])) if "items" in kw else oracle.query_leaf(kw["queries"][i])
        want, _ = O.search(oracle, forest, qv, qh, COUNT, sk, candidates=keep, want_candidates=False)
        assert got[0][i, : got[2][i]].tolist() == [a for a, _ in want], i
        assert bits(got[1][i, : got[2][i]]).tolist() == bits(np.array([b for _, b in want], np.float32)).tolist(), i
    return st, st0


# (nq, by item, filtered, AH_SEARCH_FLAG_SLICE_CANDIDATES, metric, id step): 2 slices a query, alone and beside others; 8 slices,
# most of them nearly empty; Cosine: the binary16 screen and k_search_select_screened behind the flags; ids up to 2.8 M, bitmap on
E, CASES = D.Euclidean, [(1, 0, 0, 16384), (3, 0, 0, 16384), (24, 0, 0, 16384), (3, 1, 0, 16384), (24, 0, 1, 16384), (3, 0, 0, 4096)]
CASES = [c + (E, 1) for c in CASES] + [(24, 0, 0, 16384, D.Cosine, 1), (3, 0, 0, 16384, E, 700)]


@pytest.mark.parametrize("nq,by_item,filtered,per_slice,cls,id_step", CASES,
                         ids=[f"nq{c[0]}" + "-item" * c[1] + "-filter" * c[2] + f"-{c[3]}-{c[4].__name__}-ids{c[5]}" for c in CASES])
def test_sliced_flags_keep_the_tiles_and_answer_as_the_sorted_path(nq, by_item, filtered, per_slice, cls, id_step):
    oracle, forest, index, X = built(cls, id_step=id_step)
    rng = np.random.default_rng([nq, per_slice])
    kw = {"items": rng.choice(len(X), nq, replace=False).astype(np.uint32)} if by_item else {"queries": X[rng.choice(len(X), nq)] * np.float32(0.9)}
    keep = np.arange(0, len(X), 2, dtype=np.uint32) if filtered else None
    st, st0 = both(oracle, forest, index, 30_000, keep, dict(AH_SEARCH_BITMAP=int(id_step != 1), AH_SEARCH_FLAG_SLICE_CANDIDATES=per_slice), **kw)
    assert st["rerank_tiles"] == nq and st["rerank_sorted"] == 0 and st["fallback_chunks"] == 0 and st["dedup_flag_hash"] == nq, st
    assert st0["rerank_tiles"] == 0 < st0["rerank_sorted"], st0


def test_a_slice_past_its_table_gives_the_sub_batch_up(nq=3):
    """One slice for 80 000 candidates: pass 1 counts them and leaves before a probe of the full table could spin for ever."""
    oracle, forest, index, X = built(n=40_000, trees=2)
    st, _ = both(oracle, forest, index, 80_000, None, dict(AH_SEARCH_BITMAP=0, AH_SEARCH_FLAG_SLICE_CANDIDATES=1 << 20), queries=X[:nq] * np.float32(0.9))
    assert st["fallback_select"] >= 1 and st["fallback_chunks"] >= 1 and st["rerank_tiles"] == 0, st


def test_the_default_is_off(nq=3):
    oracle, forest, index, X = built()
    assert _lib.tuning_get("AH_SEARCH_FLAG_SLICED") == (0, 0)
    with _lib.tuning(AH_SEARCH_BITMAP=0):  # the base shape with the switch left alone: the sorted path
        index.stats(reset=True)
        index.search(COUNT, queries=X[:nq], search_k=30_000, raw=True)
        assert index.stats()["rerank_tiles"] == 0 and index.stats()["rerank_sorted"] == nq, index.stats()
