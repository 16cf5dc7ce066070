"""ah_index_insert_items, ah_index_graft and ah_index_export (inserts and grafts on a resident index) and the Writer path that
uses them.  The yardstick is the host path of `Writer::build`: TreeStore with the union of the routed ids and `import_tree`.
After every step the updated index is compared with a FRESH ah_index_create_from_view of the host's store in four ways: the
export (node for node, id for id, normal rows bit for bit through the node's row), the landing node of every dataset id in
every tree, and the searches with and without candidates (ids, distance bits, counts), one of them opening every leaf."""
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
from arroy_amd.index import TreeStore  # noqa: E402

from test_gpu_index_delete import clone, host_delete, ids_of, refused, same_store  # noqa: E402

DIMS = 64
OK, DEVICE, OOM = 0, 3, 4
NONE = 0xFFFFFFFF
SMALL_N = 5000
SMALL_IDS = np.concatenate([np.arange(SMALL_N - 1, dtype=np.uint32), np.array([NONE], dtype=np.uint32)])
SEEDS = [5, 6, 7, 8, 9, 10, 11, 12]


@pytest.fixture(scope="module")
def small():
    """A 64-d Euclidean dataset of 5000 rows, ids 0 .. 4998 and 0xFFFFFFFF: what the hand-made views hang on."""
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    vecs = O.synth(3, 1, SMALL_N, DIMS)
    ds = Dataset(D.Euclidean, DIMS, SMALL_N)
    ds.upload_vectors(SMALL_IDS, vecs)
    ds.finalize()
    ds.queries = vecs[[1, 70, 700, 4000, 4999]] + np.float32(1e-3)
    ds.cand = np.sort(SMALL_IDS[::3])
    yield ds
    _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
    ds.close()


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def make_store(specs, seed=1, spread=1, same_plane=False):
    """specs: one tree each; a list of ids is a Descendants node, a pair (left, right) a split node (every second one without a
    plane, unless same_plane: then every split node has the SAME plane).  Node ids as Writer hands them out, times `spread`
    (gaps for grafted nodes to land in)."""
    g = np.random.default_rng(seed)
    s = TreeStore()
    s.roots = [s.next_id() for _ in specs]
    planes = [0]
    shared = g.standard_normal(DIMS).astype(np.float32).tobytes()

    def add(spec, nid=None):
        if isinstance(spec, tuple):
            left, right = add(spec[0]), add(spec[1])
            nid = s.next_id() if nid is None else nid
            planes[0] += 1
            vec = shared if same_plane else (g.standard_normal(DIMS).astype(np.float32).tobytes() if planes[0] % 2 else None)
            s.nodes[nid] = ("S", left, right, np.zeros(1, np.float32), vec)
        else:
            nid = s.next_id() if nid is None else nid
            s.nodes[nid] = ("D", np.array(sorted(spec), dtype=np.uint32))
        return nid
    for root, spec in zip(s.roots, specs):
        add(spec, root)
    if spread != 1:
        m = lambda i: i * spread + spread  # noqa: E731
        s.nodes = {m(k): (v if v[0] == "D" else ("S", m(v[1]), m(v[2]), v[3], v[4])) for k, v in s.nodes.items()}
        s.roots = [m(r) for r in s.roots]
    return s


def index_of(ds, store, dist=D.Euclidean):
    view, keep = store.to_view(dist, DIMS)
    return Index(ds, None, view=view), keep[4]


def host_insert(ds, store, ids, seeds, dist=D.Euclidean):
    """The host path (ArroyBuilder._incremental): route on an index of the store, union.  -> (store, touched store ids)"""
    out = clone(store)
    ids = np.asarray(ids, dtype=np.uint32)
    if ids.size == 0 or not out.roots:
        return out, []
    ix, dense = index_of(ds, out, dist)
    try:
        leaf_of = ix.route_items(ids, seeds[:len(out.roots)])
    finally:
        ix.close()
    back = {i: nid for nid, i in dense.items()}
    grown = {}
    for t in range(leaf_of.shape[0]):
        for nid in np.unique(leaf_of[t]):
            grown.setdefault(back[int(nid)], []).append(ids[leaf_of[t] == nid])
    for nid, extra in grown.items():
        out.nodes[nid] = ("D", np.union1d(out.nodes[nid][1], np.concatenate(extra)).astype(np.uint32))
    return out, sorted(grown)


def same_index(ds, ix, dense, store, seeds, dist=D.Euclidean, route=None, strict=False, search=True):
    """`ix` (store id -> node index: `dense`) against a fresh index of `store`."""
    fresh, new = index_of(ds, store, dist)
    try:
        assert sorted(dense) == sorted(new) == sorted(store.nodes)
        a, b = ix.export(), fresh.export()
        ia, ib = ix.export_info(), fresh.export_info()
        assert ia["n_trees"] == ib["n_trees"] == len(store.roots) and ia["desc_len"] == ib["desc_len"] == b["descendants"].size
        back_a, back_b = {i: nid for nid, i in dense.items()}, {i: nid for nid, i in new.items()}
        assert [back_a[int(r)] for r in a["roots"]] == [back_b[int(r)] for r in b["roots"]] == list(store.roots)
        used = np.zeros(a["nodes"].size, dtype=bool)
        for nid in store.nodes:
            x, y = a["nodes"][dense[nid]], b["nodes"][new[nid]]
            used[dense[nid]] = True
            assert x["kind"] == y["kind"] and x["has_normal"] == y["has_normal"], nid
            if x["kind"] == 1:
                assert x["count"] == y["count"], nid
                got = a["descendants"][int(x["offset"]):int(x["offset"]) + int(x["count"])]
                assert np.array_equal(got, b["descendants"][int(y["offset"]):int(y["offset"]) + int(y["count"])]), nid
                assert np.array_equal(got, store.nodes[nid][1]), nid
            else:
                assert (back_a[int(x["left"])], back_a[int(x["right"])]) == (back_b[int(y["left"])], back_b[int(y["right"])]), nid
                if x["has_normal"]:
                    assert a["normal_rows"][int(x["offset"])].tobytes() == b["normal_rows"][int(y["offset"])].tobytes(), nid
                    assert a["normal_headers"][int(x["offset"])].tobytes() == b["normal_headers"][int(y["offset"])].tobytes(), nid
        assert not a["nodes"]["kind"][~used].any()  # every other slot is free
        if strict:  # after a graft: the numbering and the blob of the fresh index
            assert dense == new and ia["n_nodes"] == ib["n_nodes"] and np.array_equal(a["roots"], b["roots"])
            assert np.array_equal(a["descendants"], b["descendants"])
            for f in ("kind", "has_normal", "left", "right", "count"):
                assert np.array_equal(a["nodes"][f], b["nodes"][f]), f
            leaves = a["nodes"]["kind"] == 1
            assert np.array_equal(a["nodes"]["offset"][leaves], b["nodes"]["offset"][leaves])
        route = ds.route_ids if route is None else route
        if len(store.roots):
            ra, rb = ix.route_items(route, seeds[:len(store.roots)]), fresh.route_items(route, seeds[:len(store.roots)])
            assert ra.shape == rb.shape == (len(store.roots), route.size)
            assert np.array_equal(np.vectorize(back_a.get)(ra), np.vectorize(back_b.get)(rb))
        if search:
            for cand in (None, ds.cand):
                for sk in (40, 10 ** 9):  # (the second opens every leaf)
                    x = ix.search(10, queries=ds.queries, search_k=sk, candidates=cand, candidates_sorted=True, raw=True)
                    y = fresh.search(10, queries=ds.queries, search_k=sk, candidates=cand, candidates_sorted=True, raw=True)
                    assert np.array_equal(x[2], y[2]) and np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes(), (sk, cand is None)
    finally:
        fresh.close()


def live(dense, store):
    return {nid: dense[nid] for nid in store.nodes}


def check_insert(ds, store, ids, seeds=SEEDS, before=None):
    """insert `ids` on an index of `store` (before: ids deleted first on the same index, so that it has holes)"""
    ids = np.array(sorted(ids), dtype=np.uint32)
    ix, dense = index_of(ds, store)
    try:
        got, want = clone(store), store
        if before is not None:
            got.apply_delta(ix.delete_items(np.array(sorted(before), dtype=np.uint32), 4), dense)
            want = host_delete(store, before, 4)
            same_store(got, want)
        delta = ix.insert_items(ids, seeds[:len(want.roots)])
        want, touched = host_insert(ds, want, ids, seeds)
        assert delta["removed"].size == 0 and np.array_equal(delta["roots"], [dense[r] for r in want.roots])
        assert [int(i) for i in delta["put_index"]] == sorted(dense[nid] for nid in touched)
        got.apply_delta(delta, dense)
        same_store(got, want)
        same_index(ds, ix, live(dense, want), want, seeds)
        return want, delta
    finally:
        ix.close()


# ---- 1. hand-made views, insert --------------------------------------------------------------------------------------------

CHAIN = [100, 101, 102]
for _d in range(1, 75):  # 74 split levels, three ids a leaf
    CHAIN = ([100 + 3 * _d, 101 + 3 * _d, 102 + 3 * _d], CHAIN)
TREE = (([1, 2, 3], [4, 5, 6]), ([7, 8], ([9, 10, 11], [12])))  # four split nodes: planes, none, plane, none

INSERTS = [
    # name, trees, inserted ids
    ("one_node_forest", [[1, 2, 3]], [0, 2, 9]),
    ("one_empty_node", [[]], [5, 6]),
    ("leaf_gets_0", [[1, 2, 3], TREE], []),
    ("leaf_gets_1", [[1, 2, 3]], [2000]),
    ("leaf_gets_63", [list(range(0, 200, 2))], list(range(1001, 1001 + 2 * 63, 2))),
    ("leaf_gets_64", [list(range(0, 200, 2))], list(range(51, 51 + 2 * 64, 2))),
    ("leaf_gets_65", [list(range(0, 200, 2))], list(range(1, 1 + 2 * 65, 2))),
    ("leaf_gets_130", [list(range(300, 500)), TREE], list(range(250, 380))),
    ("leaf_past_lds_sort", [list(range(0, 600, 3)), [7]], list(range(100, 4300))),
    ("all_already_present", [list(range(50)), TREE], [3, 4, 5, 40]),
    ("some_already_present", [list(range(0, 300, 2)), TREE], list(range(90, 130))),
    ("id_u32_max", [[5, 9], TREE], [7, NONE]),
    ("id_u32_max_present", [[5, 9, NONE], ([1], [NONE])], [NONE]),
    ("coin_nodes", [TREE, TREE, (TREE, TREE)], list(range(1000, 1400))),
    ("chain", [CHAIN, TREE], list(range(90, 400, 2))),
]


@pytest.mark.parametrize("name,specs,ids", INSERTS, ids=[h[0] for h in INSERTS])
def test_hand_made_insert(small, name, specs, ids):
    small.route_ids = SMALL_IDS[::7]
    want, delta = check_insert(small, make_store(specs), ids)
    if name == "leaf_gets_0":
        assert delta["put_index"].size == 0 and delta["desc"].size == 0
    if name == "all_already_present":
        assert delta["put_index"].size >= 2 and want.nodes[want.roots[0]][1].size == 50  # put although nothing was added
    if name == "leaf_past_lds_sort":
        assert want.nodes[want.roots[0]][1].size > 4200
    if name == "id_u32_max":
        assert int(want.nodes[want.roots[0]][1][-1]) == NONE


def test_coin_after_a_delete_left_holes(small):
    """`normal: None` nodes on the way, on an index whose delete removed nodes: the coin is keyed by the node's rank"""
    small.route_ids = SMALL_IDS[::7]
    store = make_store([TREE, (TREE, ([20, 21], [22, 23])), TREE])
    want, _ = check_insert(small, store, list(range(1000, 1300)), before=[1, 2, 3, 7, 8, 20, 21])
    assert len(want.nodes) < len(store.nodes)


def test_insert_refuses_an_id_that_is_no_row(small):
    small.route_ids = SMALL_IDS[::7]
    store = make_store([TREE, [1, 2]])
    ix, dense = index_of(small, store)
    try:
        refused(lambda: ix.insert_items([3, 4998, 4999, 6000], SEEDS[:2]), "item 4999 (position 2")
        refused(lambda: ix.insert_items([3, 3], SEEDS[:2]), "not strictly ascending")
        same_index(small, ix, dense, store, SEEDS)
    finally:
        ix.close()


# ---- 2. hand-made views, graft ---------------------------------------------------------------------------------------------

def sub_view(store, nids, dist=D.Euclidean):
    """The nodes `nids` of `store` (whole sub-trees, listed roots first) as a view of their own -> (view, keep, store id ->
    view node)."""
    sub = TreeStore()
    local = {nid: k for k, nid in enumerate(sorted(nids))}
    for nid in nids:
        nd = store.nodes[nid]
        sub.nodes[local[nid]] = nd if nd[0] == "D" else ("S", local[nd[1]], local[nd[2]], nd[3], nd[4])
    return sub, local


def graft_case(ds, base, grafts, use_new_index=True, before=None, ix_dense=None, want_map=False):
    """grafts: [(target store id or None, spec, ids of the new nodes in the order make_store hands them out)].  The host
    writes the sub-trees into a clone of `base`; the device gets them as one view."""
    want = clone(base)
    roots, members = [], []
    for target, spec, new_ids in grafts:
        t = make_store([spec], seed=7 + len(members))
        order = sorted(t.nodes)  # the root is 0, then children before parents
        rename = {0: target if target is not None else new_ids[-1]}
        for k, nid in enumerate(order[1:]):
            rename[nid] = new_ids[k]
        for nid, nd in t.nodes.items():
            want.nodes[rename[nid]] = nd if nd[0] == "D" else ("S", rename[nd[1]], rename[nd[2]], nd[3], nd[4])
        if target is None:
            want.roots.append(rename[0])
        roots.append(rename[0])
        members += [rename[nid] for nid in order]
    sub, local = sub_view(want, members)
    sub.roots = [local[r] for r in roots]
    view, keep = sub.to_view(D.Euclidean, DIMS)
    ix, dense = ix_dense if ix_dense is not None else index_of(ds, base)
    new_dense = {nid: i for i, nid in enumerate(sorted(want.nodes))}
    targets = np.array([NONE if g[0] is None else dense[g[0]] for g in grafts], dtype=np.uint32)
    new_index = np.full(len(members), NONE, dtype=np.uint32)
    for nid, k in local.items():
        if nid not in [g[0] for g in grafts]:
            new_index[k] = new_dense[nid]
    return want, ix, dense, new_dense, view, keep, targets, (new_index if use_new_index else None)


SUB3 = ([1, 2, 3], [4, 5, 6])
BASE = [TREE, ([30, 31, 32, 33], [34, 35])]   # spread 10: roots 10, 20; leaves 30, 40, 60, 70, 80, 110, 120; splits 50, 90, 100
TREE_CASES = [
    # name, grafts as (target, spec, new ids), with new_index
    ("children_before_all", [(40, SUB3, [1, 2])], True),
    ("children_between", [(40, SUB3, [41, 45])], True),
    ("children_after_all", [(40, SUB3, [500, 501])], True),
    ("children_everywhere", [(60, (SUB3, ([7, 8], [9])), [3, 55, 56, 900, 901, 902])], True),
    ("two_targets_in_one_tree", [(40, SUB3, [41, 42]), (60, ([1], ([2], [3])), [1, 700, 701, 702])], True),
    ("new_root_only", [(None, SUB3, [14, 15, 16])], True),
    ("replacing_and_new_roots", [(None, SUB3, [600, 601, 602]), (110, SUB3, [5, 6]), (None, [9, 10], [25])], True),
    ("one_node_sub_tree", [(40, [1, 2, 3, 4], [])], True),
]


@pytest.mark.parametrize("name,grafts,with_index", TREE_CASES, ids=[g[0] for g in TREE_CASES])
def test_hand_made_graft(small, name, grafts, with_index):
    small.route_ids = SMALL_IDS[::7]
    base = make_store(BASE, spread=10)
    assert base.nodes[40][0] == base.nodes[60][0] == base.nodes[110][0] == "D"
    want, ix, dense, new_dense, view, keep, targets, new_index = graft_case(small, base, grafts)
    try:
        n_old = len(base.nodes)
        got = ix.graft(view, targets, new_index, want_map=True)
        assert got.size == n_old and [int(got[dense[nid]]) for nid in base.nodes] == [new_dense[nid] for nid in base.nodes]
        same_index(small, ix, new_dense, want, SEEDS, strict=True)
        if name == "one_node_sub_tree":
            assert len(want.nodes) == n_old
    finally:
        ix.close()


def test_graft_without_new_index_appends(small):
    small.route_ids = SMALL_IDS[::7]
    base = make_store(BASE, spread=10)
    want, ix, dense, new_dense, view, keep, targets, _ = graft_case(small, base, [(40, SUB3, [500, 501]), (None, SUB3, [502, 503, 504])],
                                                                      use_new_index=False)
    try:
        assert ix.graft(view, targets, None) is None
        same_index(small, ix, new_dense, want, SEEDS, strict=True)
    finally:
        ix.close()


def test_graft_after_a_delete_left_holes_and_twice_past_the_normals_capacity(small):
    small.route_ids = SMALL_IDS[::7]
    base = make_store(BASE, spread=10)
    ix, dense = index_of(small, base)
    try:
        deleted = [1, 2, 3, 4, 5, 6, 34, 35]
        after = clone(base)
        after.apply_delta(ix.delete_items(np.array(deleted, dtype=np.uint32), 2), dense)
        same_store(after, host_delete(base, deleted, 2))
        assert len(after.nodes) < len(base.nodes) and after.nodes[80][0] == "D"
        dense = live(dense, after)
        want, ix, dense, new_dense, view, keep, targets, new_index = graft_case(
            small, after, [(80, SUB3, [40, 41])], ix_dense=(ix, dense))  # 40: an id the delete has freed
        got = ix.graft(view, targets, new_index, want_map=True)
        assert got.size == len(base.nodes)
        assert sorted(int(x) for x in got if x != NONE) == sorted(new_dense[nid] for nid in after.nodes)
        assert all((int(got[i]) == NONE) == (nid not in after.nodes) for nid, i in index_of_map(base).items())
        assert ix.export_info()["n_nodes"] == len(want.nodes)  # the holes are gone
        same_index(small, ix, new_dense, want, SEEDS, strict=True)
        # a second graft, of more planes than the first left room for: the normals move into larger arrays
        normals0 = ix.export_info()["n_normals"]
        big = [2000, 2001, 2002]
        for k in range(1, 10):  # nine split nodes, five of them with a plane
            big = (big, [2000 + 3 * k, 2001 + 3 * k, 2002 + 3 * k])
        want2, ix, dense, new_dense2, view, keep, targets, new_index = graft_case(
            small, want, [(70, big, list(range(1000, 1018)))], ix_dense=(ix, new_dense))
        ix.graft(view, targets, new_index)
        assert normals0 == 4 and ix.export_info()["n_normals"] == 9  # (room for 6 after the first graft)
        same_index(small, ix, new_dense2, want2, SEEDS, strict=True)
    finally:
        ix.close()


def index_of_map(store):
    return {nid: i for i, nid in enumerate(sorted(store.nodes))}


def test_graft_tie_break_follows_the_renumbered_nodes(small):
    """Every plane of the forest is the same plane, so the margins of a query tie across trees and the node index decides the
    order in which the descent opens them; the grafted nodes land before, between and behind the old ones."""
    small.route_ids = SMALL_IDS[::7]
    leaves = [list(range(40 * k, 40 * k + 40)) for k in range(8)]
    tree = lambda a: ((leaves[a], leaves[a + 1]), (leaves[a + 2], leaves[a + 3]))  # noqa: E731
    base = make_store([tree(0), tree(4), tree(0), tree(4)], same_plane=True, spread=10)
    target = sorted(nid for nid, nd in base.nodes.items() if nd[0] == "D")[3]
    t = make_store([(list(range(400, 420)), (list(range(420, 440)), list(range(440, 460))))], same_plane=True)
    want = clone(base)
    rename = {0: target, 1: 1, 2: target + 5, 3: 2000, 4: 2001}
    for nid, nd in t.nodes.items():
        want.nodes[rename[nid]] = nd if nd[0] == "D" else ("S", rename[nd[1]], rename[nd[2]], nd[3], nd[4])
    sub, local = sub_view(want, list(rename.values()))
    sub.roots = [local[target]]
    view, keep = sub.to_view(D.Euclidean, DIMS)
    ix, dense = index_of(small, base)
    try:
        new_dense = index_of_map(want)
        new_index = np.array([NONE if nid == target else new_dense[nid] for nid, _k in sorted(local.items(), key=lambda p: p[1])], np.uint32)
        ix.graft(view, [dense[target]], new_index)
        same_index(small, ix, new_dense, want, SEEDS, strict=True)
        fresh, _ = index_of(small, want)
        for sk in (10, 45, 90, 130, 250):  # budgets that stop the descent among the tied nodes
            x = ix.search(10, queries=small.queries, search_k=sk, raw=True)
            y = fresh.search(10, queries=small.queries, search_k=sk, raw=True)
            assert np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes() and np.array_equal(x[2], y[2]), sk
        fresh.close()
    finally:
        ix.close()


def test_graft_refusals_leave_the_index_unchanged(small):
    small.route_ids = SMALL_IDS[::7]
    base = make_store(BASE, spread=10)
    want, ix, dense, new_dense, view, keep, targets, new_index = graft_case(small, base, [(40, SUB3, [41, 45]), (None, SUB3, [46, 47, 48])])
    try:
        n_new = len(want.nodes)
        split = dense[base.roots[0]]
        bad = lambda **kw: (lambda: ix.graft(view, kw.get("targets", targets), kw.get("new_index", new_index)))  # noqa: E731
        refused(bad(targets=[len(base.nodes), NONE]), "is no node of the index")
        refused(bad(targets=[split, NONE]), "a split node")
        two = _lib.AhForestView.from_buffer_copy(view)
        refused(lambda: ix.graft(view, [dense[40], dense[40]], new_index), "target of two trees")
        ni = new_index.copy()
        first = int(np.flatnonzero(ni != NONE)[0])
        ni[first] = n_new
        refused(bad(new_index=ni), "is not below")
        ni = new_index.copy()
        a, b = np.flatnonzero(ni != NONE)[:2]
        ni[a] = ni[b]
        refused(bad(new_index=ni), "twice")
        ni = new_index.copy()
        ni[int(np.flatnonzero(new_index == NONE)[0])] = 3
        refused(bad(new_index=ni), "must be given as 0xFFFFFFFF")
        ni = new_index.copy()
        ni[first] = NONE
        refused(bad(new_index=ni), "is not below")
        same_root = (C.c_uint32 * 2)(view.roots[0], view.roots[0])  # a view that is no forest
        two.roots = C.cast(same_root, C.POINTER(C.c_uint32))
        refused(lambda: ix.graft(two, targets, new_index), "reachable twice")
        f = ix.make_filter(small.cand, sorted=True)
        refused(bad(), "live filters")
        refused(lambda: ix.insert_items([1, 2], SEEDS[:2]), "live filters")
        f.close()
        ix.suspend()
        refused(bad(), "suspended")
        refused(lambda: ix.insert_items([1, 2], SEEDS[:2]), "suspended")
        refused(lambda: ix.export(), "suspended")
        ix.resume()
        same_index(small, ix, dense, base, SEEDS)
        ix.graft(view, targets, new_index)
        same_index(small, ix, new_dense, want, SEEDS, strict=True)
        # a free slot as a target: after a delete
        ix.delete_items(np.array(ids_of(TREE), dtype=np.uint32), 4)
        refused(lambda: ix.graft(view, [new_dense[50], NONE], None), "a free slot")
    finally:
        ix.close()


# ---- 3. random forests -----------------------------------------------------------------------------------------------------

N = 20_000
WORLD_IDS = np.arange(N, dtype=np.uint32) * 3 + 7   # sparse ids


class World:
    def __init__(self, dist, split_after):
        self.dist, self.split_after = dist, split_after
        self.vecs = O.synth(21, 1, N, DIMS)
        self.ds = ds = Dataset(dist, DIMS, N)
        ds.upload_vectors(WORLD_IDS, self.vecs)
        ds.finalize()
        self.seeds = [11, 12, 13]
        forest = ds.build_forest(self.seeds, split_after=split_after)
        self.store = TreeStore()
        self.store.roots = [self.store.next_id() for _ in self.seeds]
        for t, root in enumerate(self.store.roots):
            self.store.import_tree(forest, t, root_id=root)
        forest.close()
        g = np.random.default_rng(split_after)
        self.perm = g.permutation(WORLD_IDS)
        # half of the items are in no tree yet (and their node ids are free): what an update inserts makes leaves grow
        self.store = host_delete(self.store, self.perm[N // 2:], split_after)
        ds.queries = self.vecs[g.integers(0, N, 48)] + np.float32(1e-3)
        ds.route_ids = WORLD_IDS   # every dataset id in every tree
        ds.cand = np.sort(g.choice(WORLD_IDS, N // 3, replace=False)).astype(np.uint32)

    def updated(self, share, first=0):
        """ids of an update: half of them are in the trees, half are new to them"""
        half = int(round(N * share)) // 2
        return np.sort(np.concatenate([self.perm[first:first + half], self.perm[N // 2 + first:N // 2 + first + half]]))


@pytest.fixture(scope="module", params=[("Euclidean", 8), ("Euclidean", 64), ("BinaryQuantizedEuclidean", 8),
                                        ("BinaryQuantizedEuclidean", 64)], ids=lambda p: f"{p[0]}-{p[1]}")
def world(request):
    w = World(getattr(D, request.param[0]), request.param[1])
    yield w
    _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
    w.ds.close()


def host_cycle(w, store, ids, round_seed):
    """delete -> insert -> build_subtrees -> import: one incremental build of the host path.  -> (store after the insert, store
    at the end, the overgrown nodes, their forest)"""
    out = clone(store)
    out.begin_build()
    gone = set(int(i) for i in ids)
    out.roots = sorted(out.delete_items(r, gone, w.split_after)[0] for r in out.roots)
    mid, touched = host_insert(w.ds, out, ids, w.seeds, w.dist)
    mid._next, mid._available = out._next, list(out._available)
    large = [nid for nid in touched if len(mid.nodes[nid][1]) > w.split_after]
    end = clone(mid)
    end._next, end._available = mid._next, list(mid._available)
    forest, maps = None, []
    if large:
        forest = w.ds.build_subtrees([mid.nodes[nid][1] for nid in large], [round_seed + t for t in range(len(large))], w.split_after)
        for t, nid in enumerate(large):
            end.import_tree(forest, t, root_id=nid)
            maps.append(end.last_import)
    return mid, end, large, forest, maps


def device_cycle(w, ix, dense, store, ids, host):
    """the same build on the resident index `ix`; every step is compared with the host's.  -> the new store id -> index map"""
    mid, end, large, forest, maps = host
    got = clone(store)
    got.apply_delta(ix.delete_items(ids, w.split_after), dense)
    delta = ix.insert_items(ids, w.seeds)
    got.apply_delta(delta, dense)
    same_store(got, mid)
    back = {i: nid for nid, i in dense.items()}
    assert sorted(nid for nid in (back[int(i)] for i in delta["put_index"]) if len(got.nodes[nid][1]) > w.split_after) == large
    if not large:
        return live(dense, mid)
    new_dense = index_of_map(end)
    new_index = np.full(len(forest.nodes), NONE, dtype=np.uint32)
    for t, ids_of_tree in enumerate(maps):
        for k, nid in ids_of_tree.items():
            new_index[k] = new_dense[nid]
        new_index[int(forest.roots[t])] = NONE
    ix.graft(forest.view_struct(), np.array([dense[nid] for nid in large], dtype=np.uint32), new_index)
    return new_dense


@pytest.mark.parametrize("share", [0.01, 0.10, 0.50])
def test_random_forest(world, share):
    w = world
    if w.split_after <= 8:
        assert len(w.store.nodes) > 2 * 4096  # the scans over the nodes are past one tile (4096 words)
    ids = w.updated(share)
    host = host_cycle(w, w.store, ids, 100)
    ix, dense = index_of(w.ds, w.store, w.dist)
    try:
        new_dense = device_cycle(w, ix, dense, w.store, ids, host)
        assert host[2] or share < 0.1, "no node outgrew split_after: the graft was not exercised"
        same_index(w.ds, ix, new_dense, host[1], w.seeds, w.dist, strict=True)
    finally:
        ix.close()
        if host[3] is not None:
            host[3].close()


def test_random_forest_in_several_launches(world):
    """AH_LAUNCH_MAX_ITEMS cuts the routing, the count, the scatter, the merge and the copies into several launches"""
    w = world
    ids = w.updated(0.10)
    host = host_cycle(w, w.store, ids, 100)
    ix, dense = index_of(w.ds, w.store, w.dist)
    try:
        with _lib.tuning(AH_LAUNCH_MAX_ITEMS=1000):
            new_dense = device_cycle(w, ix, dense, w.store, ids, host)
        same_index(w.ds, ix, new_dense, host[1], w.seeds, w.dist, strict=True, search=w.split_after == 8)
    finally:
        ix.close()
        if host[3] is not None:
            host[3].close()


def test_two_builds_on_one_index(world):
    """the index of build N serves build N + 1: the second build reuses the node ids the first one freed"""
    w = world
    first, second = w.updated(0.10), w.updated(0.10, first=N // 20)
    h1 = host_cycle(w, w.store, first, 100)
    h2 = host_cycle(w, h1[1], second, 200)
    ix, dense = index_of(w.ds, w.store, w.dist)
    try:
        dense = device_cycle(w, ix, dense, w.store, first, h1)
        dense = device_cycle(w, ix, dense, h1[1], second, h2)
        same_index(w.ds, ix, dense, h2[1], w.seeds, w.dist, strict=bool(h2[2]), search=w.split_after == 8)
    finally:
        ix.close()
        for h in (h1, h2):
            if h[3] is not None:
                h[3].close()


# ---- 4. allocation faults -------------------------------------------------------------------------------------------------

def sweep(call, probe, at_least, need_oom=True):
    """AH_FAIL_ALLOC_AFTER = 1, 2, ...: every allocation of `call` fails once; it returns a status, holds no memory afterwards
    and `probe` answers as before; without the fault the call succeeds.  -> what the successful call returned"""
    before = probe()
    seen = []
    for n in range(1, 200):
        live0, _ = _lib.device_cache_stats(0)
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", n)
        try:
            out, status = call(), OK
        except _lib.ArroyHipError as e:
            out, status = None, e.status
        finally:
            left = _lib.tuning_get("AH_FAIL_ALLOC_AFTER")[0]
            _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        if left > 0:  # the counter never fired: every allocation of the call has failed once
            assert status == OK
            break
        assert status in (OOM, DEVICE), (n, status)
        assert _lib.lib().ah_last_error() != b""
        assert _lib.device_cache_stats(0)[0] <= live0, n
        now = probe()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(now, before)), n
        seen.append(status)
    else:
        raise AssertionError("more than 200 allocations in one call?")
    assert len(seen) >= at_least and (OOM in seen or not need_oom), seen
    return out


def test_insert_graft_and_export_survive_every_allocation_failure(world):
    w = world
    ids = w.updated(0.10)
    host = host_cycle(w, w.store, ids, 100)
    mid, end, large, forest, maps = host
    ix, dense = index_of(w.ds, w.store, w.dist)
    try:
        q = w.ds.queries[:8]

        def probe():
            e = ix.export(normals=False)
            return ix.search(10, queries=q, search_k=500, raw=True) + (ix.route_items(w.ds.route_ids[::40], w.seeds),
                                                                       e["nodes"].view(np.uint8), e["roots"], e["descendants"])
        got = clone(w.store)
        got.apply_delta(ix.delete_items(ids, w.split_after), dense)
        got.apply_delta(sweep(lambda: ix.insert_items(ids, w.seeds), probe, 4), dense)  # work, nodes, blob, delta + host vectors
        same_store(got, mid)
        new_dense = index_of_map(end)
        new_index = np.full(len(forest.nodes), NONE, dtype=np.uint32)
        for t, ids_of_tree in enumerate(maps):
            for k, nid in ids_of_tree.items():
                new_index[k] = new_dense[nid]
            new_index[int(forest.roots[t])] = NONE
        targets = np.array([dense[nid] for nid in large], dtype=np.uint32)
        view = forest.view_struct()
        sweep(lambda: ix.graft(view, targets, new_index), probe, 6)  # work, nodes, roots, blob, records, offsets + host vectors
        e = sweep(lambda: ix.export(), lambda: (ix.route_items(w.ds.route_ids[::40], w.seeds),), 1, need_oom=False)
        assert e["nodes"].size == len(end.nodes)
        same_index(w.ds, ix, new_dense, end, w.seeds, w.dist, strict=True, search=w.split_after == 8)
    finally:
        ix.close()
        forest.close()


# ---- 5. Writer -------------------------------------------------------------------------------------------------------------

def run_writer(dist, device_insert_on, filter_alive=False):
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
        b.build()
        reader = I.Reader.open(db, 0)
        qs = vecs[[1, 500, 950, 1300]]
        snaps.append((clone(st.trees), copy.deepcopy(st.metadata), [reader.nns(10).search_k(300).by_vector(q) for q in qs],
                      reader.nns(5).by_item(st.metadata["items"][3]), st.device_inserts, st.index_uploads, st.device_deletes))
        return reader
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
    reader = build(3)
    f = reader.make_filter(range(0, 2000, 2)) if filter_alive else None
    for i in range(n0 + 300, n0 + 330):  # a build that must add two trees, with a Reader filter alive
        w.add_item(i, vecs[i])
    build(4, n_trees=7)
    assert f is None or not f._h
    for i in range(n0 + 330, n0 + 360):  # a build that drops three trees
        w.add_item(i, vecs[i])
    build(5, n_trees=4)
    for i in range(500, 520):
        assert w.del_item(i)
    build(6, n_trees=4)
    # the kept index is the index of the store: a fresh one answers the same
    view, keep = st.trees.to_view(dist, dims)
    fresh = Index(st.dataset, None, view=view)
    qs = vecs[[1, 500, 950, 1300]]
    a, b = st.index.search(10, queries=qs, search_k=300, raw=True), fresh.search(10, queries=qs, search_k=300, raw=True)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    fresh.close()
    st.index.close()
    st.dataset.close()
    return snaps


@pytest.mark.parametrize("dist_name", ["Euclidean", "BinaryQuantizedCosine"])
def test_writer_keeps_the_index_and_builds_the_same_trees(dist_name):
    dist = getattr(D, dist_name)
    dev, host = run_writer(dist, True, filter_alive=True), run_writer(dist, False)
    # the host path makes an index from the view after every build
    assert [s[4] for s in host] == [0] * 7 and [s[5] for s in host] == [1, 2, 3, 4, 5, 6, 7]
    # builds 1 - 3 keep the index (three incremental builds in a row), build 4 adds two trees on it, build 5 drops trees and
    # falls back, build 6 keeps the index again
    assert [s[4] for s in dev] == [0, 1, 2, 3, 4, 4, 5]
    assert [s[5] for s in dev] == [1, 1, 1, 1, 1, 2, 2]
    assert [s[6] for s in dev] == [s[6] for s in host]
    for k, (a, b) in enumerate(zip(dev, host)):
        same_store(a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3], k
        assert len(a[0].roots) == (5, 5, 5, 5, 7, 4, 4)[k]
