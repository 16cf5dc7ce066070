"""The tile path of mid-size submissions (AH_SEARCH_MID_TILES=1; DESIGN.md §4 "Mid-size submissions"): ids, distance bits and
counts of calls of 9 to 64 queries are the oracle's for every query and those of the same call with the switch off, and
`Index.mid_stats` says k_leaf_tiles_mid answered.  20 000 gaussian rows under 12 trees; search_k is 15 mean leaves, so the
plan's own estimate, taken from the forest's arrays on the host, admits 64 queries to the small path: only the forced overflow
overflows.  A leaf holds up to `dims` rows (four slabs at 200 dimensions).  The queries lie around five rows, 1, 2, 3, 6 and
12 per row: leaves visited by 1, 2, 3 - 4 (operands in registers), 5 - 8 and 9 - 16 queries (operands through LDS)."""
import functools

import numpy as np
import pytest

from arroy_amd import _lib, shard
from arroy_amd import distances as D
from oracle import oracle as O
from test_gpu_query_screens import bits, make, same

pytestmark = pytest.mark.gpu
COUNT, N, MAX_NQ = 10, 20_000, 64
# (metric, AH_SEARCH_SCREEN_DIFF): the dot-product screen, Euclidean's f32 rows, the difference screen
CONFIGS = [(D.Cosine, 0), (D.DotProduct, 0), (D.Euclidean, 0), (D.Manhattan, 1), (D.Euclidean, 1)]


@functools.lru_cache(maxsize=None)
def data(cls, dims):
    """(ds, oracle, forest, rows, search_k, the 64 queries) — and the admission rule of the small path, checked on the host."""
    rng = np.random.default_rng([dims, cls.metric])
    X = rng.standard_normal((N, dims)).astype(np.float32)
    ds, oracle = make(cls, X)
    forest = ds.build_forest(shard.tree_seeds(42, range(12)))
    leaves = forest.nodes["count"][forest.nodes["kind"] == 1]
    mean_leaf = forest.descendants.size / max(1, int((leaves > 0).sum()))
    sk = int(15 * mean_leaf)
    est = 1.25 * sk / mean_leaf + 2.0
    assert 4 <= est <= 128 and MAX_NQ * est <= 0.8 * 2048 and (dims < 128 or leaves.max() > 64), (mean_leaf, est, leaves.max())
    base = np.resize(np.repeat(np.arange(5), [1, 2, 3, 6, 12]), MAX_NQ)
    qs = (X[100 + 7 * base] + rng.standard_normal((MAX_NQ, dims)) * 1e-3).astype(np.float32)
    return ds, oracle, forest, X, sk, qs


@functools.lru_cache(maxsize=None)
def index_of(cls, dims, diff):
    ds, _, forest = data(cls, dims)[:3]
    with _lib.tuning(AH_SEARCH_SCREEN_DIFF=diff):
        return ds.create_index(forest)


@functools.lru_cache(maxsize=None)
def wanted(cls, dims):
    """The oracle's answers to the 64 queries, once."""
    _, oracle, forest, _, sk, qs = data(cls, dims)
    view = O.forest_view(forest)
    return [O.search(oracle, forest, *oracle.query_leaf(q), COUNT, sk, want_candidates=False, view=view)[0] for q in qs]


def at(index, mid, diff, sk, tun={}, **kw):
    with _lib.tuning(AH_SEARCH_MID_TILES=mid, AH_SEARCH_SCREEN_DIFF=diff, **tun):
        index.stats(reset=True), index.mid_stats(reset=True)
        got = index.search(COUNT, search_k=sk, raw=True, **kw)
        return got, index.stats(), index.mid_stats()


def is_oracles(got, want):
    for i, w in enumerate(want):
        assert int(got[2][i]) == len(w), i
        assert got[0][i, : len(w)].tolist() == [a for a, _ in w], i
        assert bits(got[1][i, : len(w)]).tolist() == bits(np.array([b for _, b in w], np.float32)).tolist(), i


@pytest.mark.parametrize("nq", [9, 16, 33, 64])
@pytest.mark.parametrize("dims", [40, 200])
@pytest.mark.parametrize("cls,diff", CONFIGS, ids=[c.__name__ + "-diff" * d for c, d in CONFIGS])
def test_mid_tiles_are_the_oracles_and_the_switch_changes_nothing(cls, diff, dims, nq):
    sk, qs = data(cls, dims)[4:]
    index = index_of(cls, dims, diff)
    got, st, mid = at(index, 1, diff, sk, queries=qs[:nq])
    print(cls.__name__, diff, dims, nq, mid, st)
    is_oracles(got, wanted(cls, dims)[:nq])
    ref, st0, mid0 = at(index, 0, diff, sk, queries=qs[:nq])
    same(got, ref, "switch on vs off")
    assert mid["chunks"] >= 1 and mid["queries"] == nq and mid["chunks_overflowed"] == 0 and st["fallback_chunks"] == 0, (mid, st)
    assert mid["items"] >= st["tile_units_4"] + st["tile_units_8"] + st["tile_units_16"] > 0, (mid, st)
    assert mid0 == dict.fromkeys(mid0, 0) and st0["fallback_chunks"] == 0, (mid0, st0)
    if nq >= 33:  # the n_vis classes by the unit counters: registers, LDS with 8 and with 16 sums
        assert st["tile_units_4"] > 0 and st["tile_units_8"] > 0 and st["tile_units_16"] > 0, st


EDGES = ["64 copies", "filtered", "by item", "list overflow", "nq 8", "nq 65", "max queries 12"]


@pytest.mark.parametrize("case", EDGES)
def test_edges(case, cls=D.Cosine, dims=200):
    ds, oracle, forest, X, sk, qs = data(cls, dims)
    index, kw, keep, tun = index_of(cls, dims, 0), None, None, {}
    if case == "64 copies":  # every leaf visited 64 times: units of 16 cut from one run, dedup per query
        kw, want = {"queries": np.repeat(qs[:1], 64, axis=0)}, wanted(cls, dims)[:1] * 64
    elif case == "filtered":
        keep, kw = np.arange(0, N, 2, dtype=np.uint32), {"queries": qs[:9]}
    elif case == "by item":
        kw = {"items": np.arange(300, 316, dtype=np.uint32)}
    elif case == "nq 65":
        kw = {"queries": np.concatenate([qs, qs[:1]])}
    else:
        kw = {"queries": qs[:8 if case == "nq 8" else 16]}
        tun = {"list overflow": {"AH_SEARCH_MID_ITEMS_CAP": 4}, "max queries 12": {"AH_SEARCH_MID_TILES_MAX_QUERIES": 12}}.get(case, {})
    if case != "64 copies":
        leaf = (lambda i: oracle.item_leaf(int(kw["items"][i]))) if "items" in kw else (lambda i: oracle.query_leaf(kw["queries"][i]))
        want = [O.search(oracle, forest, *leaf(i), COUNT, sk, candidates=keep, want_candidates=False)[0] for i in range(len(next(iter(kw.values()))))]
    got, st, mid = at(index, 1, 0, sk, tun=tun, candidates=keep, **kw)
    print(case, mid, st)
    is_oracles(got, want)
    same(got, at(index, 0, 0, sk, candidates=keep, **kw)[0], "switch on vs off")
    if case == "list overflow":
        assert mid["chunks_overflowed"] >= 1 and mid["chunks"] == 0 and st["fallback_chunks"] >= 1, (mid, st)
    elif case in ("nq 8", "nq 65", "max queries 12"):
        assert mid == dict.fromkeys(mid, 0), mid
    else:
        assert mid["chunks"] >= 1 and mid["chunks_overflowed"] == 0 and st["fallback_chunks"] == 0, (mid, st)
        assert case != "64 copies" or (st["tile_units_16"] > 0 and st["tile_units_4"] + st["tile_units_8"] == 0), st
