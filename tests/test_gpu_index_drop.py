"""ah_index_drop_trees (`delete_extra_trees`, src/writer.rs:631-655, on a resident index) and the Writer path that uses it
(ArroyBuilder.device_drop).  The yardstick is the host's store: `clone(store)`, index.roots_after_drop and TreeStore.delete_tree.
The device's delta applied to a clone must leave exactly that store (same_store), and the index after the drop is compared with
a FRESH ah_index_create_from_view of that store (same_index of the insert tests: node for node, id for id, normal rows through
the node's row, the landing node of every dataset id in every tree, searches with and without candidates), plus the one thing
same_index leaves open after a call that keeps free slots: the descendants blob is the fresh index's blob, byte for byte.

Every id of every hand-made view is a row of the dataset (ids below 300), because the comparison searches: the CHAIN and SIZES
shapes of the delete tests are restated here with such ids."""
import copy
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

from arroy_amd import Dataset, Index, _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from arroy_amd import index as I  # noqa: E402
from arroy_amd.index import TreeStore, roots_after_drop  # noqa: E402

import audit_model as M  # noqa: E402
from test_gpu_index_delete import clone, host_delete, refused, same_store  # noqa: E402
from test_gpu_index_insert import host_insert, index_of, index_of_map, live, make_store, same_index, sweep  # noqa: E402

DIMS = 64
N_ROWS = 300
NONE = 0xFFFFFFFF
INVALID = 5
IDS = list(range(N_ROWS))
SEEDS = [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20]


@pytest.fixture(scope="module")
def small():
    """The 64-d Euclidean dataset of 300 rows of the delete tests, ids 0 .. 299, with what same_index asks of a dataset."""
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    vecs = O.synth(3, 1, N_ROWS, DIMS)
    ds = Dataset(D.Euclidean, DIMS, N_ROWS)
    ds.upload_vectors(np.arange(N_ROWS, dtype=np.uint32), vecs)
    ds.finalize()
    ds.queries = vecs[[1, 70, 150, 299]] + np.float32(1e-3)
    ds.cand = np.arange(0, N_ROWS, 3, dtype=np.uint32)
    ds.route_ids = np.arange(N_ROWS, dtype=np.uint32)
    yield ds
    _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
    ds.close()


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def host_drop(store, n_drop, sort_roots=False):
    """-> (the store after `delete_extra_trees`, the store ids of the nodes it deleted); sort_roots: what AH_DROP_SORT_ROOTS
    promises, the roots ascending after a call that dropped something (a call that drops nothing does nothing)"""
    out = clone(store)
    out.roots, dropped = roots_after_drop(out.roots, n_drop)
    for root in dropped:
        out.delete_tree(root)
    if sort_roots and dropped:
        out.roots.sort()
    return out, sorted(set(store.nodes) - set(out.nodes))


def drop_first(store, chosen):
    """The roots of `store` reordered so that `delete_extra_trees` of len(chosen) trees drops exactly the roots `chosen`:
    swap_remove(0) takes the first root, then what was the last, the one before it, ..."""
    chosen = list(chosen)
    rest = [r for r in store.roots if r not in chosen]
    store.roots = chosen[:1] + rest + chosen[:0:-1]
    assert sorted(roots_after_drop(store.roots, len(chosen))[1]) == sorted(chosen)
    return store


def same_blob(ds, ix, store, dist=D.Euclidean):
    """the lists of the surviving Descendants nodes in ascending node order with their exact lengths: the blob of a fresh index"""
    fresh, _ = index_of(ds, store, dist)
    try:
        a, b = ix.export(normals=False), fresh.export(normals=False)
        assert a["descendants"].tobytes() == b["descendants"].tobytes()
        leaves = a["nodes"]["kind"] == 1
        assert np.array_equal(a["nodes"]["offset"][leaves], b["nodes"]["offset"][b["nodes"]["kind"] == 1])
    finally:
        fresh.close()


def check_drop(ds, store, n_drop, sort_roots=False, seeds=SEEDS, tuning=None, search=True):
    """drop on an index of `store`; -> (the host's store afterwards, the delta, the index, store id -> node index)"""
    ix, dense = index_of(ds, store)
    try:
        want, gone = host_drop(store, n_drop, sort_roots)
        if tuning:
            with _lib.tuning(**tuning):
                delta = ix.drop_trees(n_drop, sort_roots=sort_roots)
        else:
            delta = ix.drop_trees(n_drop, sort_roots=sort_roots)
        assert delta["put_index"].size == 0 and delta["put"].size == 0 and delta["desc"].size == 0
        assert delta["removed"].dtype == np.uint32 and delta["removed"].tolist() == sorted(dense[nid] for nid in gone)
        assert delta["roots"].tolist() == [dense[r] for r in want.roots]
        got = clone(store)
        got.apply_delta(delta, dense)
        same_store(got, want)
        same_index(ds, ix, live(dense, want), want, seeds, search=search)
        same_blob(ds, ix, want)
        info = ix.export_info()
        assert info["n_nodes"] == len(store.nodes) and info["n_trees"] == len(want.roots)  # node indices are stable
        return want, delta, ix, dense
    except BaseException:
        ix.close()
        raise


def leaf(first, n):
    return [(first + k) % N_ROWS for k in range(n)]


A, B = [1, 2, 3], [4, 5, 6]
TREE = (([1, 2, 3], [4, 5, 6]), ([7, 8], ([9, 10, 11], [12])))  # four split nodes: plane, none, plane, none
CHAIN = [0, 1, 2]
for _d in range(1, 75):  # 74 split levels, three ids a leaf: ids 0 .. 224
    CHAIN = ([3 * _d, 3 * _d + 1, 3 * _d + 2], CHAIN)


# ---- 1. the roots ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sort_roots", [False, True], ids=["swap_remove_order", "sorted"])
@pytest.mark.parametrize("n_drop", range(0, 9))
def test_root_order(small, n_drop, sort_roots):
    store = make_store([[10 * t, 10 * t + 1] for t in range(6)])
    store.roots = [store.roots[i] for i in (3, 0, 5, 1, 4, 2)]  # (not ascending to begin with)
    want, delta, ix, dense = check_drop(small, store, n_drop, sort_roots)
    ix.close()
    assert len(want.roots) == max(0, 6 - n_drop) and len(want.nodes) == len(want.roots)  # 7 and 8 clamp
    r = store.roots
    if n_drop == 0:
        assert want.roots == r and delta["removed"].size == 0
    if n_drop == 4:
        assert want.roots == (sorted([r[2], r[1]]) if sort_roots else [r[2], r[1]])
    if sort_roots and n_drop:
        assert want.roots == sorted(want.roots)
    elif n_drop == 2:
        assert want.roots == [r[4], r[1], r[2], r[3]] and want.roots != sorted(want.roots)


@pytest.mark.parametrize("sort_roots", [False, True], ids=["swap_remove_order", "sorted"])
def test_dropping_nothing_changes_nothing(small, sort_roots):
    store = make_store([TREE, [7, 8, 9], (A, B)])
    store.roots = store.roots[::-1]
    ix, dense = index_of(small, store)
    try:
        before = ix.export()
        live0 = _lib.device_cache_stats(0)[0]
        delta = ix.drop_trees(0, sort_roots=sort_roots)
        assert _lib.device_cache_stats(0)[0] == live0
        # (the current roots, also with AH_DROP_SORT_ROOTS: the call does nothing)
        assert delta["roots"].tolist() == [dense[r] for r in store.roots]
        assert all(delta[k].size == 0 for k in ("removed", "put_index", "put", "desc"))
        after = ix.export()
        assert sorted(before) == sorted(after) and all(before[k].tobytes() == after[k].tobytes() for k in before)
        assert ix.footprint()["free_slots"] == 0 and ix.compact()["moved"] == 0  # still the index of its creation
    finally:
        ix.close()


# ---- 2. the walk -----------------------------------------------------------------------------------------------------------

WALKS = [
    # name, trees (the first one is dropped), n_drop
    ("chain_of_74_levels", [CHAIN, TREE], 1),
    ("single_descendants_root", [[1, 2, 3], TREE, [7, 8]], 1),
    ("split_without_a_normal", [((A, B), [7, 8]), TREE, (TREE, TREE)], 1),   # the dropped root has `normal: None`
    ("chain_and_its_neighbours", [TREE, CHAIN, (A, B), CHAIN, [9]], 3),      # drops trees 0, 4 and 3; a chain survives
    ("every_tree", [CHAIN, TREE], 2),
]


@pytest.mark.parametrize("name,specs,n_drop", WALKS, ids=[w[0] for w in WALKS])
def test_walk(small, name, specs, n_drop):
    store = make_store(specs)
    want, delta, ix, dense = check_drop(small, store, n_drop)
    ix.close()
    if name == "chain_of_74_levels":
        assert delta["removed"].size == 149 and len(want.nodes) == 9
    if name == "split_without_a_normal":
        assert store.nodes[store.roots[0]][4] is None and any(nd[0] == "S" and nd[4] is None for nd in want.nodes.values())
    if name == "every_tree":
        assert not want.nodes and not want.roots


# ---- 3. the copy -----------------------------------------------------------------------------------------------------------

def test_every_surviving_list_moves_by_another_amount(small):
    """lists of 0, 1, 63, 64, 65, 130 and 192 ids stay; in front of each of them in node order lies a dropped list of another
    length (the roots are numbered first, so the lists of the dropped split tree lie behind them all)"""
    sizes = [0, 1, 63, 64, 65, 130, 192]
    dropped = [leaf(5, 2), leaf(20, 3), leaf(40, 5), leaf(50, 64), leaf(60, 7), leaf(70, 129), leaf(80, 11), (leaf(90, 1), leaf(95, 70))]
    specs = []
    for k, d in enumerate(dropped):
        specs.append(d)
        if k < len(sizes):
            specs.append(leaf(17 * k, sizes[k]))
    store = make_store(specs)
    drop_first(store, store.roots[0::2])
    want, delta, ix, dense = check_drop(small, store, len(dropped))
    try:
        assert sorted(len(nd[1]) for nd in want.nodes.values()) == sizes and len(want.roots) == len(sizes)
        ex = ix.export(normals=False)
        old, _ = index_of(small, store)
        moved = [int(old.export(normals=False)["nodes"]["offset"][dense[r]]) - int(ex["nodes"]["offset"][dense[r]]) for r in sorted(want.roots)]
        old.close()
        assert len(set(moved)) == len(moved) and min(moved) > 0, moved
    finally:
        ix.close()


# ---- 4. past one scan tile and one launch ------------------------------------------------------------------------------------

def test_more_nodes_than_a_scan_tile_in_launches_of_seven(small):
    n_trees = 4000
    specs = [([t % N_ROWS], [(t + 1) % N_ROWS]) if t % 16 == 0 else [t % N_ROWS] for t in range(n_trees)]
    store = make_store(specs)
    assert len(store.nodes) > 4096 + 256  # kScanTile, and the dropped nodes alone are not a multiple of it
    seeds = list(range(100, 100 + n_trees))
    want, delta, ix, dense = check_drop(small, store, n_trees // 2, seeds=seeds, tuning={"AH_LAUNCH_MAX_ITEMS": 7})
    ix.close()
    assert len(want.roots) == n_trees // 2 and delta["removed"].size == len(store.nodes) - len(want.nodes) > n_trees // 2


# ---- 5. holes already present -------------------------------------------------------------------------------------------------

def test_drop_after_a_delete_then_insert_and_graft(small):
    specs = [TREE, (TREE, ([20, 21], [22, 23])), leaf(100, 40), TREE, (A, B), (leaf(200, 30), leaf(240, 30))]
    store = make_store(specs)
    ix, dense = index_of(small, store)
    fresh = None
    try:
        gone = [1, 2, 3, 7, 8, 20, 21, 240]
        mid = clone(store)
        mid.apply_delta(ix.delete_items(np.array(gone, dtype=np.uint32), 4), dense)
        same_store(mid, host_delete(store, gone, 4))
        holes = len(store.nodes) - len(mid.nodes)
        assert holes >= 4 and ix.footprint()["free_slots"] == holes
        want, dropped = host_drop(mid, 2)
        got = clone(mid)
        got.apply_delta(ix.drop_trees(2), dense)
        same_store(got, want)
        same_index(small, ix, live(dense, want), want, SEEDS)
        same_blob(small, ix, want)
        assert ix.footprint()["free_slots"] == holes + len(dropped)
        # the same insert on the dropped index and on a fresh index of the store
        fresh, fdense = index_of(small, want)
        ids = np.arange(30, 300, 7, dtype=np.uint32)
        seeds = SEEDS[:len(want.roots)]
        a, b = clone(want), clone(want)
        da, db = ix.insert_items(ids, seeds), fresh.insert_items(ids, seeds)
        a.apply_delta(da, dense)
        b.apply_delta(db, fdense)
        same_store(a, b)
        same_store(a, host_insert(small, want, ids, SEEDS)[0])
        assert da["desc"].tobytes() == db["desc"].tobytes() and da["put_index"].size == db["put_index"].size > 0
        same_index(small, ix, live(dense, a), a, SEEDS)
        # ... and the same graft: a new tree behind every node; afterwards both are the fresh index of the host's store
        sub = make_store([(leaf(0, 20), (leaf(20, 20), leaf(40, 20)))], seed=9)
        view, keep = sub.to_view(D.Euclidean, DIMS)
        base = max(a.nodes) + 1
        end = clone(a)
        for nid, nd in sub.nodes.items():
            end.nodes[base + nid] = nd if nd[0] == "D" else ("S", base + nd[1], base + nd[2], nd[3], nd[4])
        end.roots.append(base + sub.roots[0])
        ix.graft(view, [_lib.NEW_ROOT])
        fresh.graft(view, [_lib.NEW_ROOT])
        new_dense = index_of_map(end)
        same_index(small, ix, new_dense, end, SEEDS, strict=True)
        same_index(small, fresh, new_dense, end, SEEDS, strict=True, search=False)
    finally:
        ix.close()
        if fresh is not None:
            fresh.close()


# ---- 6. waste and audit -----------------------------------------------------------------------------------------------------

def test_footprint_audit_and_compaction_after_a_drop(small):
    """every tree holds every row of the dataset once, so that the audit can call the index valid"""
    specs = [(IDS[:100], (IDS[100:200], IDS[200:])), IDS, ((IDS[:50], IDS[50:150]), (IDS[150:151], IDS[151:])), (IDS[:299], IDS[299:]),
             ((IDS[:10], IDS[10:20]), ((IDS[20:30], IDS[30:40]), IDS[40:]))]
    store = drop_first(make_store(specs), [0, 3, 4])  # (the roots are the store ids 0 .. 4)
    want, delta, ix, dense = check_drop(small, store, 3)
    try:
        gone = sorted(set(store.nodes) - set(want.nodes))
        planes = sum(1 for nid in gone if store.nodes[nid][0] == "S" and store.nodes[nid][4] is not None)
        assert len(gone) == 5 + 3 + 9 and planes >= 2
        fp = ix.footprint()
        assert fp["n_nodes"] == len(store.nodes) and fp["free_slots"] == len(gone)
        assert fp["n_normals"] - fp["live_normals"] == planes
        assert fp["desc_len"] == 2 * N_ROWS
        rep = ix.audit(trees=True)
        assert rep == M.model_of_export(ix.export(normals=False), IDS, ix.export_info()["n_normals"], trees=True)
        assert rep["valid"] == 1 and rep["floating"] == 0 and all(rep[c] == 0 for c in M.CLASSES)
        assert rep["nodes_in_use"] == rep["nodes_reached"] == len(want.nodes)
        assert M.plain_stats(rep) == M.store_stats(want)
        assert [t["root"] for t in rep["tree_stats"]] == [dense[r] for r in want.roots]
        # the compaction reclaims the free slots and the orphaned rows: the export of a fresh index of the store
        stats, new_of_old = ix.compact(want_map=True)
        assert stats["moved"] == 1 and stats["nodes_after"] == len(want.nodes) and stats["normals_after"] == fp["live_normals"]
        new_dense = index_of_map(want)
        assert {nid: int(new_of_old[i]) for nid, i in live(dense, want).items()} == new_dense
        assert all(int(new_of_old[dense[nid]]) == NONE for nid in gone)
        same_index(small, ix, new_dense, want, SEEDS, strict=True)
        fresh, _ = index_of(small, want)
        a, b = ix.export(), fresh.export()
        fresh.close()
        assert sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() for k in a), [k for k in a if a[k].tobytes() != b[k].tobytes()]
        fp = ix.footprint()
        assert fp["free_slots"] == 0 and fp["n_normals"] == fp["live_normals"]
    finally:
        ix.close()


# ---- 7. built forests, two metrics ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dist_name", ["Euclidean", "BinaryQuantizedCosine"])
def test_built_forest(dist_name):
    dist = getattr(D, dist_name)
    n, dims, seeds = 900, 24, [31, 32, 33, 34, 35, 36]
    vecs = np.random.default_rng(11).standard_normal((n, dims)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint32) * 2 + 1
    ds = Dataset(dist, dims, n)
    ix = fresh = None
    try:
        ds.upload_vectors(ids, vecs)
        ds.finalize()
        forest = ds.build_forest(seeds, split_after=dims)
        store = TreeStore()
        store.roots = [store.next_id() for _ in seeds]
        for t, root in enumerate(store.roots):
            store.import_tree(forest, t, root_id=root)
        forest.close()
        view, keep = store.to_view(dist, dims)
        ix, dense = Index(ds, None, view=view), keep[4]
        want, gone = host_drop(store, 4)
        assert want.roots == [store.roots[2], store.roots[1]]
        got = clone(store)
        got.apply_delta(ix.drop_trees(4), dense)
        same_store(got, want)
        view, keep = want.to_view(dist, dims)
        fresh, fdense = Index(ds, None, view=view), keep[4]
        back_a, back_b = {i: nid for nid, i in dense.items()}, {i: nid for nid, i in fdense.items()}
        queries = vecs[[0, 13, 450, 899]] + np.float32(1e-3)
        for kw in (dict(queries=queries), dict(items=ids[[5, 600]])):
            a, b = ix.search(10, search_k=300, raw=True, **kw), fresh.search(10, search_k=300, raw=True, **kw)
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
            assert int(a[2].min()) == 10
        ra, rb = ix.route_items(ids, seeds[:2]), fresh.route_items(ids, seeds[:2])
        assert ra.shape == rb.shape == (2, n)
        assert np.array_equal(np.vectorize(back_a.get)(ra), np.vectorize(back_b.get)(rb))
        assert ix.export(normals=False)["descendants"].tobytes() == fresh.export(normals=False)["descendants"].tobytes()
    finally:
        for x in (ix, fresh):
            if x is not None:
                x.close()
        ds.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_index_unchanged(small):
    store = make_store([TREE, (A, B), [7, 8, 9], TREE])
    ix, dense = index_of(small, store)
    try:
        L = _lib.lib()
        h = C.c_void_p(1)
        assert L.ah_index_drop_trees(ix._h, 1, 0, None) == INVALID and b"out_delta" in L.ah_last_error()
        assert L.ah_index_drop_trees(None, 1, 0, C.byref(h)) == INVALID and b"index is NULL" in L.ah_last_error() and not h.value
        for flags in (2, 3, 0x80000000):
            h = C.c_void_p(1)
            assert L.ah_index_drop_trees(ix._h, 1, flags, C.byref(h)) == INVALID and b"flags" in L.ah_last_error() and not h.value
        f = ix.make_filter(small.cand, sorted=True)
        refused(lambda: ix.drop_trees(1), "live filters")
        same_index(small, ix, dense, store, SEEDS, search=False)
        f.close()
        ix.suspend()
        refused(lambda: ix.drop_trees(1), "suspended")
        ix.resume()
        same_index(small, ix, dense, store, SEEDS)
        assert ix.footprint()["free_slots"] == 0
        with pytest.raises(ValueError):
            ix.drop_trees(-1)
        # the same call goes through once nothing stands against it
        want, _ = host_drop(store, 1)
        got = clone(store)
        got.apply_delta(ix.drop_trees(1), dense)
        same_store(got, want)
        same_index(small, ix, live(dense, want), want, SEEDS)
    finally:
        ix.close()


# ---- 9. allocation failures -----------------------------------------------------------------------------------------------

def test_drop_survives_every_allocation_failure(small):
    store = make_store([TREE, CHAIN, leaf(100, 130), (A, B), (leaf(0, 64), leaf(64, 65)), TREE])
    ix, dense = index_of(small, store)
    try:
        def probe():
            e = ix.export(normals=False)
            return ix.search(10, queries=small.queries, search_k=200, raw=True) + (
                ix.route_items(small.route_ids, SEEDS[:len(e["roots"])]), e["nodes"].view(np.uint8), e["roots"], e["descendants"])
        # the work block, nodes, roots, ranks, blob, the removed list + the host's vectors
        delta = sweep(lambda: ix.drop_trees(3), probe, 6)
        want, _ = host_drop(store, 3)
        got = clone(store)
        got.apply_delta(delta, dense)
        same_store(got, want)
        same_index(small, ix, live(dense, want), want, SEEDS)
        same_blob(small, ix, want)
    finally:
        ix.close()


# ---- 10. Writer -------------------------------------------------------------------------------------------------------------

def run_writer(dist, device_drop_on, device_insert_on=True):
    """the build sequence of the insert tests' run_writer (builds 5 and 6 ask for fewer trees than there are), device_drop as
    given on every build"""
    dims, n0 = 24, 900
    g = np.random.default_rng(5)
    vecs = g.standard_normal((n0 + 800, dims)).astype(np.float32)
    db = I.Database(dist)
    w = I.Writer(db, 0, dims)
    st = w._st
    snaps = []

    def build(k, n_trees=5):
        b = w.builder(random.Random(40 + k)).n_trees(n_trees)
        b.device_insert = device_insert_on
        if device_drop_on is not None:
            b.device_drop = device_drop_on
        b.build()
        reader = I.Reader.open(db, 0)
        qs = vecs[[1, 500, 950, 1300]]
        snaps.append((clone(st.trees), copy.deepcopy(st.metadata), [reader.nns(10).search_k(300).by_vector(q) for q in qs],
                      reader.nns(5).by_item(st.metadata["items"][3]), st.device_inserts, st.index_uploads, st.device_deletes,
                      st.device_drops))
    for i in range(n0):
        w.add_item(i, vecs[i])
    build(0)
    for i in range(n0, n0 + 300):   # add, replace, delete
        w.add_item(i, vecs[i])
    for i in range(0, 50):
        w.add_item(i, vecs[n0 + 300 + i])
    for i in range(100, 200):
        assert w.del_item(i)
    build(1)
    for i in range(200, 400):       # delete only
        assert w.del_item(i)
    build(2)
    for i in range(400, 500):       # replace only
        w.add_item(i, vecs[n0 + 400 + i - 400])
    build(3)
    for i in range(n0 + 300, n0 + 330):  # a build that must add two trees
        w.add_item(i, vecs[i])
    build(4, n_trees=7)
    for i in range(n0 + 330, n0 + 360):  # a build that drops three trees
        w.add_item(i, vecs[i])
    build(5, n_trees=4)
    for i in range(500, 520):
        assert w.del_item(i)
    build(6, n_trees=4)
    same_as_fresh(st, dist, dims, vecs[[1, 500, 950, 1300]])
    st.index.close()
    st.dataset.close()
    return snaps


def same_as_fresh(st, dist, dims, qs):
    """the kept index is the index of the store: a fresh one answers the same"""
    view, keep = st.trees.to_view(dist, dims)
    fresh = Index(st.dataset, None, view=view)
    try:
        a, b = st.index.search(10, queries=qs, search_k=300, raw=True), fresh.search(10, queries=qs, search_k=300, raw=True)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
        assert int(a[2].min()) == 10
    finally:
        fresh.close()


@pytest.mark.parametrize("dist_name", ["Euclidean", "BinaryQuantizedCosine"])
def test_writer_drops_trees_on_the_kept_index_and_builds_the_same_trees(dist_name):
    dist = getattr(D, dist_name)
    dev, host = run_writer(dist, True), run_writer(dist, False, device_insert_on=False)
    assert [s[5] for s in host] == [1, 2, 3, 4, 5, 6, 7] and [s[7] for s in host] == [0] * 7
    # one upload, at the first build; build 5 drops its three trees on the index, build 6 has nothing to drop
    assert [s[5] for s in dev] == [1] * 7
    assert [s[7] for s in dev] == [0, 0, 0, 0, 0, 1, 1]
    assert [s[4] for s in dev] == [0, 1, 2, 3, 4, 5, 6]
    for k, (a, b) in enumerate(zip(dev, host)):
        same_store(a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3], k
        assert len(a[0].roots) == (5, 5, 5, 5, 7, 4, 4)[k]


def test_writer_default_still_falls_back_when_trees_are_dropped():
    """device_drop is off unless asked for: the counts of today"""
    dev = run_writer(D.Euclidean, None)  # (the attribute is left as the builder makes it)
    assert [s[5] for s in dev] == [1, 1, 1, 1, 1, 2, 2] and [s[7] for s in dev] == [0] * 7
    assert [s[4] for s in dev] == [0, 1, 2, 3, 4, 4, 5]
    assert I.ArroyBuilder(I.Writer(I.Database(D.Euclidean), 0, 24), random.Random(1)).device_drop is False


@pytest.mark.parametrize("change", ["one_new_item", "no_item_at_all"])
def test_writer_drops_trees_in_a_build_that_deletes_nothing(change):
    """one_new_item: the only updated id is in no tree (the delete that follows the drop finds nothing, and sorts the roots).
    no_item_at_all: nothing is updated, no delete follows: the drop itself leaves the roots sorted (AH_DROP_SORT_ROOTS)."""
    dims, n0 = 24, 900
    vecs = np.random.default_rng(6).standard_normal((n0 + 1, dims)).astype(np.float32)
    runs = []
    for on in (True, False):
        db = I.Database(D.Euclidean)
        w = I.Writer(db, 0, dims)
        st = w._st
        for i in range(n0):
            w.add_item(i, vecs[i])
        b = w.builder(random.Random(3)).n_trees(6)
        b.device_drop = on
        b.build()
        first = list(st.trees.roots)
        if change == "one_new_item":
            w.add_item(n0, vecs[n0])
        b = w.builder(random.Random(4)).n_trees(2)
        b.device_drop = on
        b.build()
        reader = I.Reader.open(db, 0)
        runs.append((clone(st.trees), copy.deepcopy(st.metadata), [reader.nns(10).search_k(300).by_vector(q) for q in vecs[[1, 500, n0]]],
                     st.index_uploads, st.device_drops, st.device_deletes))
        assert st.trees.roots == sorted(roots_after_drop(first, 4)[0]) == sorted([first[2], first[1]])
        if on:
            same_as_fresh(st, D.Euclidean, dims, vecs[[1, 500, n0]])
        st.index.close()
        st.dataset.close()
    dev, host = runs
    same_store(dev[0], host[0])
    assert dev[1] == host[1] and dev[2] == host[2]
    assert (dev[3], dev[4]) == (1, 1) and (host[3], host[4]) == (2, 0)
    assert dev[5] == (1 if change == "one_new_item" else 0)
