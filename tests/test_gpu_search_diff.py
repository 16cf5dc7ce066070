"""The difference screen in the tile pass of ah_search_batch (AH_SEARCH_SCREEN_DIFF=1): Euclidean / Manhattan
sub-batches scored on the binary16 rows by k_leaf_tiles_diff16, the survivors in f32 by k_search_select_diff.  Every call
runs under AH_SCREEN_VERIFY=1; ids, distance bits and counts are those of the same call at 0 and, for the picked queries, the
oracle's; `Index.search_diff_stats` says whether the stage answered, overflowed or switched itself off."""
import functools

import numpy as np
import pytest

from arroy_amd import _lib, shard
from arroy_amd import distances as D
from oracle import oracle as O
from test_diff_screen_bound_cpu import intervals, pruning_inputs
from test_gpu_query_screens import bits, make, same, search_checked

pytestmark = pytest.mark.gpu
METRICS = pytest.mark.parametrize("cls", [D.Euclidean, D.Manhattan], ids=["euclidean", "manhattan"])
COUNT, SK = 10, 600


@functools.lru_cache(maxsize=None)
def built(cls, dims, case="gaussian"):
    """(ds, oracle, forest, index, rows): a few thousand rows under 12 trees, the index made with the switch on (the binary16 copy)."""
    X = pruning_inputs("offset 100" if case == "offset 100" else "gaussian", dims)[0][:3000].copy()
    if case == "near-duplicates":  # as in test_gpu_diff_screen.py: everything closer together than delta
        rng = np.random.default_rng(dims)
        X = (X[0] + rng.standard_normal((3000, dims)) * 1e-5).astype(np.float32)
    if case == "non-finite":
        X[17, 0] = np.float32(1e6)
    ds, oracle = make(cls, X)
    forest = ds.build_forest(shard.tree_seeds(42, range(12)))
    with _lib.tuning(AH_SEARCH_SCREEN_DIFF=1):
        return ds, oracle, forest, ds.create_index(forest), X


def queries_near(X, nq, rng):
    """nq queries around five rows, 1, 2, 3, 6, 12, 1, ... of them per row: leaves visited by 1, 2, 3-4, 5-8 and more queries."""
    base = np.resize(np.repeat(np.arange(5), [1, 2, 3, 6, 12]), nq)
    return (X[100 + 7 * base] + rng.standard_normal((nq, X.shape[1])) * 1e-3).astype(np.float32)


def at(index, ds, diff, count, sk, **kw):
    """One search at AH_SEARCH_SCREEN_DIFF=diff under verify: the raw answer, Index.stats, search_diff_stats, verify counters."""
    tun = kw.pop("tun", {})
    with _lib.tuning(AH_SCREEN_VERIFY=1, AH_SEARCH_SCREEN_DIFF=diff, **tun):
        index.stats(reset=True), index.search_diff_stats(reset=True), ds.query_screen_verify(reset=True)
        got = index.search(count, search_k=sk, raw=True, **kw)
        return got, index.stats(), index.search_diff_stats(), ds.query_screen_verify()


# (nq, tunables, by item, filtered): Flat of one query, Flat with per_query, small tiles, Big2D behind k_units_small with the
# fused-flag selection, Big2D behind the leaf scan; ItemList, Small2D; by item; under a uniform filter that keeps half the ids
LADDER = [(1, {}, 0, 0), (4, {}, 0, 0), (8, {}, 0, 0), (40, {}, 0, 0), (200, {}, 0, 0), (4, {"AH_SEARCH_MULTI": 0}, 0, 0),
          (4, {"AH_SEARCH_ITEM_LIST": 0}, 0, 0), (8, {}, 1, 0), (8, {}, 0, 1)]


@METRICS
@pytest.mark.parametrize("dims", [32, 72, 200])
@pytest.mark.parametrize("nq,tun,by_item,filtered", LADDER, ids=[f"nq{c[0]}" + "".join(f"-{k[10:]}0" for k in c[1]) +
                                                                  "-item" * c[2] + "-filter" * c[3] for c in LADDER])
def test_tile_ladder(cls, dims, nq, tun, by_item, filtered):
    ds, oracle, forest, index, X = built(cls, dims)
    rng = np.random.default_rng([dims, nq])
    qs = queries_near(X, nq, rng)
    kw = {"items": rng.choice(len(X), nq, replace=False).astype(np.uint32)} if by_item else {"queries": qs}
    keep = np.arange(0, len(X), 2, dtype=np.uint32) if filtered else None
    ref, st0, d0, v0 = at(index, ds, 0, COUNT, SK, tun=tun, candidates=keep, **kw)
    assert d0["chunks_screened"] == 0 and v0["checked"] == 0 and st0["rerank_screened"] == 0, (d0, v0, st0)
    got, st, d, v = at(index, ds, 1, COUNT, SK, tun=tun, candidates=keep, **kw)
    print(cls.__name__, dims, nq, tun, st, d, v)
    same(got, ref, "setting 1 vs setting 0")
    assert v["violations"] == 0 and v["checked"] > 0, v
    assert d["queries"] == nq == st["rerank_screened"] and d["chunks_screened"] == 1 and d["chunks_overflowed"] == 0, (d, st)
    assert st["fallback_chunks"] == 0 and d["survivors"] == st["screen_survivors"] >= COUNT * nq, (d, st)
    if not by_item and not filtered:  # the n_vis classes by the unit counters: > 8 visits, 5 - 8, at most 4
        assert (nq == 200 or st["tile_units_4"] > 0) and (nq < 40 or st["tile_units_16"] > 0) and (nq != 40 or st["tile_units_8"] > 0), st
    for i in {0, nq - 1}:  # the oracle's answer on the same forest
        qv, qh = oracle.item_leaf(int(kw["items"][i])) if by_item else oracle.query_leaf(qs[i])
        want, _ = O.search(oracle, forest, qv, qh, COUNT, SK, candidates=keep, want_candidates=False)
        assert got[0][i, : got[2][i]].tolist() == [a for a, _ in want], i
        assert bits(got[1][i, : got[2][i]]).tolist() == bits(np.array([b for _, b in want], np.float32)).tolist(), i


@METRICS
@pytest.mark.parametrize("case", ["gaussian", "offset 100"])
def test_pruning_happens(cls, case, dims=200, nq=8):
    """The numpy restatement (test_diff_screen_bound_cpu.intervals) over the same 3000 rows, every row a candidate of query 0,
    leaves 11 (gaussian) and 150 (offset 100) of them for Euclidean, 10 and 294 for Manhattan: 0.3 - 9.8 %, under a quarter,
    so the ceiling of a half is asserted on the GPU."""
    ds, oracle, forest, index, X = built(cls, dims, case)
    qs = queries_near(X, nq, np.random.default_rng(3))
    lo, hi = intervals(cls.metric, X, qs[0])[0]["lanes"]  # (every row: a superset of the query's candidates)
    share = float((lo <= np.sort(hi)[COUNT - 1]).sum()) / len(X)
    st, v = search_checked(index, ds, oracle, forest, COUNT, 2000, queries=qs, AH_SEARCH_SCREEN_DIFF=1)
    print(cls.__name__, case, "restated share", share, st)
    assert st["rerank_screened"] == nq and COUNT * nq <= st["screen_survivors"], st
    if share < 0.25:
        assert st["screen_survivors"] <= nq * 2000 // 2, (st, v)  # (a query collects at least search_k = 2000 candidates)


@METRICS
def test_overflow_takes_the_sorted_path_and_eight_switch_the_stage_off(cls):
    ds, oracle, forest, index, X = built(cls, 32, "near-duplicates")
    q = X[5:6].copy()
    ref = at(index, ds, 0, COUNT, 2500, queries=q)[0]
    for i in range(9):  # more than 1024 candidates within delta of the k-th; the ninth call finds the stage off
        got, st, d, v = at(index, ds, 1, COUNT, 2500, queries=q)
        same(got, ref)
        assert v["violations"] == 0 and st["rerank_sorted"] == (i < 8 or cls is D.Manhattan), (i, st, v)  # (off: Euclidean's f32 tiles)
        assert (d["chunks_screened"], d["chunks_overflowed"], d["switched_off"]) == ((1, 1, i == 7) if i < 8 else (0, 0, 1)), (i, d)
    search_checked(index, ds, oracle, forest, COUNT, 2500, queries=q, AH_SEARCH_SCREEN_DIFF=1)  # off: the oracle's all the same


@METRICS
def test_non_finite_screen_value_takes_the_exact_path(cls):
    ds, oracle, forest, index, X = built(cls, 32, "non-finite")
    q, sk = X[18:19], 12 * len(X)  # (every row is a candidate, row 17 with its entry of 1e6 — inf in binary16 — among them)
    ref = at(index, ds, 0, COUNT, sk, queries=q)[0]
    got, st, d, v = at(index, ds, 1, COUNT, sk, queries=q)
    same(got, ref)
    assert st["fallback_non_finite"] == 1 and d["queries"] == 0 and d["chunks_overflowed"] == 0 and d["switched_off"] == 0, (st, d)
    search_checked(index, ds, oracle, forest, COUNT, sk, queries=q, AH_SEARCH_SCREEN_DIFF=1)
