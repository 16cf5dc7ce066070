"""Every width ladder end to end, bit for bit against the oracle (tests/width_ladder.py states the ladders and
tests/test_width_ladder_cpu.py that these widths take every rung of them).

One case = one metric at one width: ~4000 rows of make_data (its duplicates and its zero row), 9 trees with split_after = 300 (leaves
of more than one 128-row slab, k_descend_multi for the small calls), sparse ascending ids in every other case.  Each case is two
tests: scans, re-ranks and splits; forest, searches through every descent x re-rank pair, and routing.  The stats of the library
say which kernel served a call, so a fall-back cannot stand in for the path under test.

A batched re-rank that the row-major kernels take is never screened (api.hip: rerank_batch_chunk), so the screens of Cosine and
DotProduct are asserted on the same lists with the row-major path off.  1-bit margins are small integers and the reference orders
equal keys of two trees by node id, so the wave and block descents hand nearly every 1-bit query that meets such keys where search_k
cuts the leaves to the sequential queue (by design: test_gpu_parity.py, ..._equal_keys_between_trees).  The 1-bit cases therefore
assert those two descents on an index of the first tree alone, where no second tree can hold an equal key."""
import numpy as np
import pytest

import test_gpu_parity as P
import width_ladder as W
from oracle import oracle as O
from test_gpu_parity import assert_bit_equal, check_forest_valid, make_data

pytestmark = pytest.mark.gpu

from arroy_amd import Index, _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from arroy_amd._lib import tuning  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _imports():
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    P.D, P.O = D, O  # make_data / check_forest_valid live in test_gpu_parity and use its lazily imported modules


N_ROWS, SPLIT_AFTER, COUNT, SEARCH_K = 4000, 300, 20, 1500
SEEDS = [101, 102, 103, 104, 105, 106, 107, 2**63 + 8, 109]  # 9 trees: more than one wave has octets for

F32_CASES = [(m, d) for d in W.F32_WIDTHS for m in ((0, 2) if d not in W.F32_WIDTHS_ALL_METRICS else (0, 1, 2, 3))]
# all three 1-bit metrics at three widths; elsewhere BinaryQuantizedCosine and, in turn, one of the other two
BQ_CASES = [(m, d) for i, d in enumerate(W.BQ_WIDTHS)
            for m in ((4, 5, 6) if d in W.BQ_WIDTHS_ALL_METRICS else (4 + i % 2, 6))]
CASES = F32_CASES + BQ_CASES
IDS = [f"{D.BY_METRIC[m].__name__}-{d}" for m, d in CASES]


def case_data(metric, dims):
    ids = None
    if CASES.index((metric, dims)) % 2:
        ids = np.sort(np.random.default_rng(dims).choice(60_000, N_ROWS, replace=False)).astype(np.uint32)
    return make_data(D.BY_METRIC[metric], N_ROWS, dims, seed=7000 + 13 * metric + dims, ids=ids)


def same_raw(a, b, what):
    assert np.array_equal(a[2], b[2]), f"{what}: counts differ for queries {np.flatnonzero(a[2] != b[2])[:8]}"
    assert np.array_equal(a[0], b[0]), f"{what}: ids differ for queries {np.flatnonzero((a[0] != b[0]).any(axis=1))[:8]}"
    bad = np.flatnonzero((a[1].view(np.uint32) != b[1].view(np.uint32)).any(axis=1))
    assert bad.size == 0, f"{what}: distances differ for queries {bad[:8]}"


def rows_of(a, pick):
    return tuple(x[pick] for x in a)


# ---- scans, re-ranks, splits --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric,dims", CASES, ids=IDS)
def test_scan_rerank_split(metric, dims):
    ds, oracle, vecs, ids = case_data(metric, dims)
    n = N_ROWS
    what = f"m={metric} d={dims}"
    rng = np.random.default_rng(dims + metric)
    q = rng.standard_normal(dims).astype(np.float32)
    qv, qh = oracle.query_leaf(q)
    iv, ih = oracle.item_leaf(7)
    sub = np.sort(rng.choice(n, 300, replace=False)).astype(np.uint32)
    want_q, want_i = oracle.distances(qv, qh), oracle.distances(iv, ih)
    # distances: the built-in grid, a grid of 8 blocks (the grid-stride loop runs), Manhattan by the octet kernel as well
    settings = [{}, {"AH_SCAN_BLOCKS": 8}] + ([{"AH_SCAN_BLOCKS": 8, "AH_MANHATTAN_ROWS": 0}, {"AH_MANHATTAN_ROWS": 0}] if metric == 1 else [])
    for tun in settings:
        with tuning(**tun):
            assert_bit_equal(ds.distances(query=q), want_q, f"{what} scan by vector {tun}")
            assert_bit_equal(ds.distances(item=int(ids[7])), want_i, f"{what} scan by item {tun}")
            assert_bit_equal(ds.distances(item=int(ids[7]), ids=ids[sub]), want_i[sub], f"{what} gather {tun}")
            assert_bit_equal(ds.distances(query=q, ids=ids[sub]), want_q[sub], f"{what} gather by vector {tun}")
    # re-rank of one list: short and long, by the one-launch selection and by the general one
    for rows in (np.sort(rng.choice(n, 40, replace=False)).astype(np.uint32), np.sort(rng.choice(n, 3000, replace=False)).astype(np.uint32)):
        ei, ed = oracle.rerank(qv, qh, rows, COUNT)
        for small in (1, 0):
            with tuning(AH_RERANK_SMALL=small):
                oi, od = ds.rerank(COUNT, query=q, sorted_ids=ids[rows])
            assert list(oi) == [int(x) for x in ei], f"{what} rerank of {len(rows)} small={small}"
            assert_bit_equal(od, ed, f"{what} rerank of {len(rows)} small={small}")
    # batched re-rank: 48 lists with >= 3 candidates per stored row (row-run kernel), 6 lists with between 2 and 3 (pair per slot)
    screened_metric = metric in (2, 3)
    for nq in (48, 6):
        qs = rng.standard_normal((nq, dims)).astype(np.float32)
        sizes = [int(x) for x in rng.integers(n // 8, n, nq)] if nq > 6 else [n * 5 // 12] * nq
        if nq > 6:
            sizes[0], sizes[1] = n, 0  # every row, and an empty list
        assert sum(sizes) >= 2 * n and (sum(sizes) >= 3 * n) == (nq > 6)  # the thresholds of the two row-major kernels (batch.hip)
        lists = [np.sort(rng.choice(n, m, replace=False)).astype(np.uint32) for m in sizes]
        id_lists = [ids[l] for l in lists]
        res = {}
        # row-major whenever legal; then query-major, where the certified screen of Cosine / DotProduct applies: int8 first,
        # binary16 only, unscreened (AH_SCREEN8 = 1: the int8 copy is kept whatever the data)
        for name, tun in (("row-major", dict(AH_RERANK_INVERT=1)), ("row-major, screens off", dict(AH_RERANK_INVERT=1, AH_RERANK_SCREEN=0)),
                          ("int8 first", dict(AH_RERANK_INVERT=0, AH_RERANK_SCREEN=1, AH_RERANK_SCREEN8=1)),
                          ("binary16", dict(AH_RERANK_INVERT=0, AH_RERANK_SCREEN=1, AH_RERANK_SCREEN8=0)),
                          ("unscreened", dict(AH_RERANK_INVERT=0, AH_RERANK_SCREEN=0, AH_RERANK_SCREEN8=0)),
                          ("unscreened, int8 allowed", dict(AH_RERANK_INVERT=0, AH_RERANK_SCREEN=0, AH_RERANK_SCREEN8=1))):
            with tuning(AH_SCREEN8=1, **tun):
                ds.rerank_stats(reset=True)
                res[name] = ds.rerank_batch(qs, id_lists, COUNT)
                st = ds.rerank_stats()
            screen_on = screened_metric and name in ("int8 first", "binary16")
            assert (st["queries_screened"] > 0) == screen_on, (what, nq, name, st)
            assert (st["chunks_int8"] + st["chunks_int8_retried"] > 0) == (screened_metric and name == "int8 first"), (what, nq, name, st)
        for name in res:
            same_raw(res["row-major"], res[name], f"{what} rerank_batch of {nq}: row-major vs {name}")
        oi, od, oc = res["row-major"]
        for i in (0, 2, nq - 1):
            v, h = oracle.query_leaf(qs[i])
            ci, cd = oracle.rerank(v, h, lists[i], COUNT)
            assert int(oc[i]) == len(ci) and list(oi[i, : oc[i]]) == [int(x) for x in ci], f"{what} rerank_batch of {nq}, list {i}"
            assert_bit_equal(od[i, : oc[i]], cd, f"{what} rerank_batch of {nq}, list {i}")
        if nq > 6:
            assert oc[1] == 0
    # one split of a 12-id sample, the sides and margins of every row
    sample = rng.choice(n, 12, replace=False).astype(np.uint32)
    nv, nh = ds.create_split(ids[sample])
    env, enh = oracle.create_split(sample)
    assert nv.tobytes() == env.tobytes(), f"{what} normal"
    assert_bit_equal(nh, enh, f"{what} normal header")
    sides, n_left, margins = ds.split_sides(nv, nh)
    es, enl, em = oracle.split_sides(env, enh)
    assert_bit_equal(margins, em, f"{what} margins")
    assert np.array_equal(sides, es) and n_left == enl, f"{what} sides"
    part = np.sort(rng.choice(n, 777, replace=False)).astype(np.uint32)
    sides, n_left, margins = ds.split_sides(nv, nh, sorted_ids=ids[part])
    es, enl, em = oracle.split_sides(env, enh, rows=part)
    assert_bit_equal(margins, em, f"{what} margins of a subset")
    assert np.array_equal(sides, es) and n_left == enl, f"{what} sides of a subset"


# ---- forest, search, routing ----------------------------------------------------------------------------------------------

def make_queries(vecs, dims, rng, unrelated=50):
    """12 exact copies of one vector (their descents and leaves are the same: units of 12 visits), 6 of another, 2 near pairs, 50
    unrelated queries and a stored vector three items hold: 73 queries, past the threshold of the int8 stage (65).
    (1-bit cases ask for 150 unrelated ones: their margins are small integers, so most queries meet equal keys of two trees where
    search_k cuts the leaves, and the wave and block descents leave those to the sequential queue by design.)"""
    a, b = rng.standard_normal((2, dims)).astype(np.float32)
    qs = [a] * 12 + [b] * 6
    for _ in range(2):
        base = vecs[rng.integers(len(vecs))]
        qs += [base + rng.standard_normal(dims).astype(np.float32) * np.float32(1e-3) for _ in range(2)]
    qs += list(rng.standard_normal((unrelated, dims)).astype(np.float32))
    qs.append(vecs[1])
    return np.ascontiguousarray(np.stack(qs), dtype=np.float32)


def check_against_oracle(oracle, forest, view, leaves, got, picks, what, cand=None, search_k=SEARCH_K):
    oi, od, oc = got
    for i in picks:
        qv, qh = leaves[i]
        want, _ = O.search(oracle, forest, qv, qh, COUNT, search_k, 0, cand, candidates_sorted=cand is not None, want_candidates=False, view=view)
        assert list(oi[i, : oc[i]]) == [a for a, _ in want], f"{what}: ids of query {i}"
        assert_bit_equal(od[i, : oc[i]], [d for _, d in want], f"{what}: distances of query {i}")


def oracle_forest_in_the_numbering_of(forest, trees, stride, vector_bytes):
    """The oracle's trees as one caller-owned forest: its nodes, its normals ([header][vector] records of ah_header_size +
    ah_vector_size bytes: no pad word) and its Descendants, under the node ids of `forest` (a queue pops equal keys by node id, so
    only the same numbering has to give the same answers)."""
    nodes = np.zeros(len(forest.nodes), dtype=forest.nodes.dtype)
    normals, desc, n_bytes, n_desc = [], [], 0, 0
    for t, tree in enumerate(trees):
        stack = [(int(forest.roots[t]), tree.root)]
        while stack:
            g, o = stack.pop()
            kind, has_normal, left, right, offset, count, depth = tree.nodes[o]
            assert int(forest.nodes[g]["kind"]) == kind
            if kind == 1:
                nodes[g] = (1, 0, 0, t, 0, 0, n_desc, count, depth)
                desc.append(tree.descendants[offset:offset + count])
                n_desc += count
            else:
                gl, gr = int(forest.nodes[g]["left"]), int(forest.nodes[g]["right"])
                nodes[g] = (2, has_normal, 0, t, gl, gr, n_bytes if has_normal else 0, 0, depth)
                if has_normal:
                    normals.append(np.frombuffer(tree.normals[offset:offset + stride], dtype=np.uint8))
                    n_bytes += stride
                stack += [(gl, left), (gr, right)]
    import types
    return types.SimpleNamespace(n_trees=len(trees), roots=np.array(forest.roots, dtype=np.uint32), nodes=nodes,
                                 normals=np.concatenate(normals) if normals else np.zeros(0, np.uint8), normal_stride=stride,
                                 _hdr_off=0, _vec_off=stride - vector_bytes,
                                 descendants=np.ascontiguousarray(np.concatenate(desc), dtype=np.uint32))


DESCENTS = (("block", dict(AH_SEARCH_WAVE=1, AH_SEARCH_BLOCK_MAX_QUERIES=1024), "descent_block"),
            ("wave", dict(AH_SEARCH_WAVE=1, AH_SEARCH_BLOCK_MAX_QUERIES=0), "descent_wave_small"),
            ("octet", dict(AH_SEARCH_WAVE=0, AH_SEARCH_BLOCK_MAX_QUERIES=0), "descent_octet_lds"),
            ("octet, block allowed", dict(AH_SEARCH_WAVE=0, AH_SEARCH_BLOCK_MAX_QUERIES=1024), "descent_octet_lds"))
TIERS = ("descent_block", "descent_wave_small", "descent_wave_big", "descent_octet_lds", "descent_octet_global")
RERANKS = [(f"tiles={t} screen={s} screen8={s8}", dict(AH_SEARCH_TILES=t, AH_SEARCH_SCREEN=s, AH_SEARCH_SCREEN8=s8))
           for t in (1, 0) for s in (1, 0) for s8 in (1, 0)]


@pytest.mark.parametrize("metric,dims", CASES, ids=IDS)
def test_forest_search_route(metric, dims):
    ds, oracle, vecs, ids = case_data(metric, dims)
    n = N_ROWS
    what = f"m={metric} d={dims}"
    one_bit = metric >= 4
    has_tiles = metric in (0, 2, 3)       # the leaf tiles exist for Euclidean, Cosine and DotProduct (search.hip: `tiles`)
    has_screen = metric in (2, 3)         # ... and their certified screens for Cosine and DotProduct
    rng = np.random.default_rng(1000 + dims + metric)
    # the forest under the default margin mode
    forest = ds.build_forest(SEEDS, split_after=SPLIT_AFTER)
    check_forest_valid(forest, n, ids=ids)
    trees = [oracle.build_tree(SPLIT_AFTER, s) for s in SEEDS]
    for t, tree in enumerate(trees):
        assert forest.canonical(t) == tree.canonical(), f"{what}: tree {t} differs from the oracle"
    assert forest.stats["margin_evaluations"] == sum(t.margin_evals for t in trees), what
    assert forest.stats["screen_violations"] == 0, what
    assert int(forest.nodes["count"][forest.nodes["kind"] == 1].max()) > 128, "no leaf of more than one slab"
    view = O.forest_view(forest)
    queries = make_queries(vecs, dims, rng, unrelated=150 if one_bit else 50)
    nq = len(queries)
    assert nq >= 65
    leaves = [oracle.query_leaf(q) for q in queries]
    # (the oracle's side of the premise: exact copies open the same leaves and get the same candidates)
    first = O.search(oracle, forest, *leaves[0], COUNT, SEARCH_K, view=view)
    for i in (5, 11):
        again = O.search(oracle, forest, *leaves[i], COUNT, SEARCH_K, view=view)
        assert again[0] == first[0] and np.array_equal(again[1], first[1])
    with tuning(AH_SCREEN8=1):  # the int8 copy is made and kept whatever the data
        index = ds.create_index(forest)
        res, stats = {}, {}
        for dname, dtun, dcounter in DESCENTS:
            for rname, rtun in RERANKS:
                with tuning(**dtun, **rtun):
                    index.stats(reset=True)
                    res[dname, rname] = index.search(COUNT, queries=queries, search_k=SEARCH_K, raw=True)
                    st = stats[dname, rname] = index.stats()
                tiles_on, screen_on = has_tiles and rtun["AH_SEARCH_TILES"] == 1, has_screen and rtun["AH_SEARCH_TILES"] == 1 and rtun["AH_SEARCH_SCREEN"] == 1
                assert st["fallback_chunks"] == 0 and st["queries"] == nq, (what, dname, rname, st)
                assert sum(st[k] for k in TIERS) == nq, (what, dname, rname, st)
                if one_bit and dname != "octet":
                    # search_k (tripled for these metrics, reader.rs:330-335) cuts the leaves where two trees hold equal integer
                    # keys for nearly every query: handed to the sequential queue by design.  The uncut call below asserts the
                    # wave and block descents themselves.
                    assert st["descent_octet_lds"] + st["descent_octet_global"] > 0, (what, dname, rname, st)
                else:
                    assert st[dcounter] > 0, (what, dname, rname, dcounter, st)
                if tiles_on:
                    assert st["rerank_tiles"] == nq and st["tile_units_16"] > 0 and st["tile_units_8"] > 0 and st["tile_units_4"] > 0, (what, dname, rname, st)
                else:
                    assert st["rerank_sorted"] == nq and st["rerank_tiles"] == 0, (what, dname, rname, st)
                assert st["rerank_screened"] == (nq if screen_on else 0), (what, dname, rname, st)
                assert (st["rerank_screened8"] > 0) == (screen_on and rtun["AH_SEARCH_SCREEN8"] == 1), (what, dname, rname, st)
        default = index.search(COUNT, queries=queries, search_k=SEARCH_K, raw=True)
        for key in res:
            same_raw(default, res[key], f"{what}: default vs {key}")
        check_against_oracle(oracle, forest, view, leaves, default, range(nq), f"{what} search")
        for i in range(1, 12):  # the copies: equal answers
            assert np.array_equal(default[0][i], default[0][0]) and default[1][i].tobytes() == default[1][0].tobytes()
        # further call shapes: five queries, one query (single-unit tiles, KF = 24), two equal queries (KF = 12)
        # (two copies, each descent writing its own units: units of one visit; placed by one block for both: units of two visits)
        for name, pick, extra in (("first five", list(range(5)), {}), ("one query", [30], {}), ("one of the copies", [0], {}),
                                  ("two copies", [0, 1], {}), ("two copies, shared units", [0, 1], dict(AH_SEARCH_MULTI_OWN_UNITS=0)),
                                  ("the stored duplicate", [nq - 1], {})):
            for rname, rtun in RERANKS[:3] if has_screen else RERANKS[:1]:
                with tuning(**rtun, **extra):
                    index.stats(reset=True)
                    got = index.search(COUNT, queries=queries[pick], search_k=SEARCH_K, raw=True)
                    st = index.stats()
                same_raw(rows_of(default, pick), got, f"{what}: {name} as one call ({rname})")
                assert st["fallback_chunks"] == 0, (what, name, st)
                if has_tiles:
                    assert st["descent_multi"] == len(pick) and st["rerank_tiles"] == len(pick), (what, name, rname, st)
                if has_screen:
                    assert st["rerank_screened"] == (len(pick) if rtun["AH_SEARCH_SCREEN"] else 0), (what, name, rname, st)
                if has_tiles and extra:  # equal queries open the same leaves: every unit holds both visits (leaf_tile16's KF = 12)
                    assert st["tile_visits"] == 2 * (st["tile_units_4"] + st["tile_units_8"] + st["tile_units_16"]) > 0, (what, name, rname, st)
                if has_screen and len(pick) == 1 and rtun["AH_SEARCH_SCREEN"]:  # units of one visit (KF = 24)
                    assert st["tile_visits"] == st["tile_units_4"] > 0, (what, name, rname, st)
        # under a candidate filter that keeps a third of the ids
        cand = np.sort(rng.choice(ids, n // 3, replace=False)).astype(np.uint32)
        index.stats(reset=True)
        filtered = index.search(COUNT, queries=queries, search_k=SEARCH_K, candidates=cand, candidates_sorted=True, raw=True)
        assert index.stats()["fallback_chunks"] == 0
        some = range(0, nq, 3) if one_bit else range(nq)  # (the oracle's 1-bit search is the slow side of a case)
        check_against_oracle(oracle, forest, view, leaves, filtered, some, f"{what} filtered search", cand=cand)
        with tuning(AH_SEARCH_TILES=0):
            same_raw(filtered, index.search(COUNT, queries=queries, search_k=SEARCH_K, candidates=cand, candidates_sorted=True, raw=True),
                     f"{what}: filtered, tiles vs sorted")
        # by item
        item_rows = rng.choice(n, nq, replace=False).astype(np.uint32)
        item_rows[:12] = item_rows[0]
        item_rows[-1] = 1
        by_item = index.search(COUNT, items=ids[item_rows], search_k=SEARCH_K, raw=True)
        check_against_oracle(oracle, forest, view, [oracle.item_leaf(int(r)) for r in item_rows], by_item, some, f"{what} search by item")
        if one_bit:
            # the same trees as the CPU built them, normals without the pad word: the same answers as the GPU's own forest
            stride = 4 * O.header_floats(metric) + O.vector_bytes(metric, dims)
            assert trees[0].stride == stride == _lib.lib().ah_header_size(metric) + _lib.lib().ah_vector_size(metric, dims)
            theirs = oracle_forest_in_the_numbering_of(forest, trees, stride, O.vector_bytes(metric, dims))
            by_view = Index(ds, None, view=O.forest_view(theirs))
            for dname, dtun, _ in DESCENTS[:3]:
                with tuning(**dtun):
                    same_raw(default, by_view.search(COUNT, queries=queries, search_k=SEARCH_K, raw=True), f"{what}: the oracle's forest by view, {dname}")
            same_raw(by_item, by_view.search(COUNT, items=ids[item_rows], search_k=SEARCH_K, raw=True), f"{what}: the oracle's forest by view, by item")
            # The wave and block descents themselves: equal keys matter only between the leaves of two octets, and the octets of
            # both kernels split the TREES of a query, so with the first tree alone no query can be handed back for them.
            # search_k = 0 is the reference's default (count x trees x 3 for these metrics: 60 ids, a few leaves, far inside
            # the kernels' capacities).  The 1-bit arm of descent_margin runs with the query leaf in LDS, pad word included, on the
            # GPU's tree and on the oracle's through the view.  (AH_SEARCH_SMALL_GATE = 0: whatever the host's estimate of the
            # leaves says, the call starts on the kernel the setting names.)
            one = ds.build_forest(SEEDS[:1], split_after=SPLIT_AFTER)
            assert one.canonical(0) == trees[0].canonical()
            one_view = O.forest_view(one)
            theirs_one = oracle_forest_in_the_numbering_of(one, trees[:1], stride, O.vector_bytes(metric, dims))
            first40 = list(range(40))  # (the copies, the near pairs and 18 unrelated queries)
            single = {}
            for ix_name, ix in (("own tree", ds.create_index(one)), ("the oracle's tree by view", Index(ds, None, view=O.forest_view(theirs_one)))):
                for dname, dtun, dcounter in DESCENTS[:3]:
                    with tuning(AH_SEARCH_SMALL_GATE=0, **dtun):
                        ix.stats(reset=True)
                        single[ix_name, dname] = ix.search(COUNT, queries=queries[first40], search_k=0, raw=True)
                        st = ix.stats()
                    served = f"{what}: one tree, {ix_name}, {dname}: " + ", ".join(f"{k}={v}" for k, v in st.items() if v)
                    assert st["fallback_chunks"] == 0 and sum(st[k] for k in TIERS) == len(first40), served
                    assert st[dcounter] > 0, served
                    same_raw(single["own tree", "block"], single[ix_name, dname], f"{what}: one tree, own tree by block vs {ix_name} by {dname}")
                ix.close()
            check_against_oracle(oracle, one, one_view, leaves, single["own tree", "block"], first40, f"{what} search of one tree", search_k=0)
            route_rows = np.sort(rng.choice(n, 200, replace=False)).astype(np.uint32)
            assert np.array_equal(by_view.route_items(ids[route_rows], SEEDS), index.route_items(ids[route_rows], SEEDS))
            by_view.close()
        # routing of 500 items through the trees
        rows = np.sort(rng.choice(n, 500, replace=False)).astype(np.uint32)
        assert np.array_equal(index.route_items(ids[rows], SEEDS), O.route_items(oracle, forest, rows, SEEDS)), f"{what} routing"
