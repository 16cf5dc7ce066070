"""ah_index_delete_items (`delete_items_from_trees`, src/writer.rs:978-1114, on a resident index), ah_index_suspend / _resume and
the Writer path that uses them.  The yardstick is TreeStore.delete_items, the host restatement of `delete_items_in_file` that
the reference's incremental snapshots pin: the delta of the device, applied to a copy of the store, must leave exactly the
nodes and roots the host walk leaves; searches and routings on the updated index must equal those of a fresh index made from
the store after the delete."""
import copy
import random

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

from arroy_amd import Dataset, Index, _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from arroy_amd import index as I  # noqa: E402
from arroy_amd.index import TreeStore  # noqa: E402

DIMS = 64
OK, DEVICE, OOM = 0, 3, 4


@pytest.fixture(scope="module")
def small():
    """A 64-d Euclidean dataset of 300 rows: what the hand-made views hang on (a delete reads no row)."""
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    ds = Dataset(D.Euclidean, DIMS, 300)
    ds.upload_vectors(np.arange(300, dtype=np.uint32), O.synth(3, 1, 300, DIMS))
    ds.finalize()
    yield ds
    _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
    ds.close()


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def make_store(specs, dist=D.Euclidean, seed=1):
    """specs: one tree each; a list of ids is a Descendants node, a pair (left, right) a split node (every second one without a
    plane).  Roots get their ids first, then every tree its nodes, children before parents (as Writer does)."""
    g = np.random.default_rng(seed)
    s = TreeStore()
    hs, vs = dist.header_size(), dist.vector_size(DIMS)
    s.roots = [s.next_id() for _ in specs]
    planes = [0]

    def add(spec, nid=None):
        if isinstance(spec, tuple):
            left, right = add(spec[0]), add(spec[1])
            nid = s.next_id() if nid is None else nid
            planes[0] += 1
            vec = g.integers(0, 256, vs, dtype=np.uint8).tobytes() if planes[0] % 2 else None
            s.nodes[nid] = ("S", left, right, g.standard_normal(hs // 4).astype(np.float32), vec)
        else:
            nid = s.next_id() if nid is None else nid
            s.nodes[nid] = ("D", np.array(sorted(spec), dtype=np.uint32))
        return nid
    for root, spec in zip(s.roots, specs):
        add(spec, root)
    return s


def clone(store):
    c = TreeStore()
    c.nodes = {k: (("D", v[1].copy()) if v[0] == "D" else v) for k, v in store.nodes.items()}
    c.roots = list(store.roots)
    return c


def same_store(a, b):
    assert a.roots == b.roots, (a.roots, b.roots)
    assert sorted(a.nodes) == sorted(b.nodes), (sorted(set(a.nodes) ^ set(b.nodes))[:10])
    for nid, x in a.nodes.items():
        y = b.nodes[nid]
        assert x[0] == y[0], nid
        if x[0] == "D":
            assert x[1].dtype == y[1].dtype == np.uint32 and np.array_equal(x[1], y[1]), (nid, x[1][:8], y[1][:8])
        else:
            assert x[1:3] == y[1:3] and np.array_equal(x[3], y[3]) and x[4] == y[4], nid


def host_delete(store, ids, split_after):
    out = clone(store)
    gone = set(int(i) for i in ids)
    out.roots = sorted(out.delete_items(r, gone, split_after)[0] for r in out.roots)
    return out


def device_delete(ds, store, ids, split_after, dist=D.Euclidean):
    """-> (the store after the device's delta, the updated index, store id -> node index of that index)"""
    view, keep = store.to_view(dist, DIMS)
    ix = Index(ds, None, view=view)
    out = clone(store)
    out.apply_delta(ix.delete_items(np.array(sorted(ids), dtype=np.uint32), split_after), keep[4])
    return out, ix, keep[4]


def check(ds, store, ids, split_after):
    got, ix, _ = device_delete(ds, store, ids, split_after)
    ix.close()
    want = host_delete(store, ids, split_after)
    same_store(got, want)
    return want


def ids_of(spec):
    return [i for part in spec for i in ids_of(part)] if isinstance(spec, tuple) else list(spec)


# ---- 1. hand-made views: one case per rule -------------------------------------------------------------------------------

A, B = [1, 2, 3], [4, 5, 6]
CHAIN = [100, 101, 102]
for _d in range(1, 75):  # 74 split levels, three ids a leaf
    CHAIN = ([100 + 3 * _d, 101 + 3 * _d, 102 + 3 * _d], CHAIN)
SIZES = (list(range(1000, 1063)), (list(range(2000, 2064)), (list(range(3000, 3065)), (list(range(4000, 4130)), list(range(5000, 5192))))))

HAND = [
    # name, trees, deleted ids, split_after
    ("left_empty", [(A, B)], A, 4),
    ("right_empty", [(A, B)], B, 4),
    ("both_empty_right_survives", [(A, B)], A + B, 4),
    ("merge_at_split_after", [(A, B)], [3, 6], 4),
    ("one_more_stays_split", [(A, B)], [3], 4),
    ("none_and_empty", [((A, B), [7, 8])], [7, 8], 4),
    ("empty_and_none", [([7, 8], (A, B))], [7, 8], 4),
    ("cascade_three_levels", [((([1, 9], [2, 10]), [3, 11]), [4, 12])], [9, 10, 11, 12], 4),
    ("cascade_stops_half_way", [((([1, 9], [2, 10]), [3, 11]), [4, 12, 13, 14])], [9, 10, 11], 4),
    ("single_root_emptied", [[1, 2]], [1, 2], 4),
    ("root_replaced_order_changes", [(A, B), ([7, 8, 9], [10, 11, 12])], A, 4),
    ("chain", [CHAIN], [100 + 3 * d + k for d in range(0, 75, 2) for k in (0, 2)] + [103, 104, 105], 4),
    ("chain_collapses", [CHAIN], [100 + 3 * d + k for d in range(75) for k in (0, 1)], 4),
    ("chain_all", [CHAIN], ids_of(CHAIN), 4),
    ("leaf_sizes", [SIZES], [1062, 2063, 3064, 4129, 5000], 64),
    ("leaf_sizes_more", [SIZES], list(range(1000, 1063)) + list(range(2001, 2064, 2)) + [3000, 4064, 5191], 64),
    ("id_u32_max", [([5, 0xFFFFFFFF, 9], [6, 0xFFFFFFFE, 7])], [0xFFFFFFFF], 4),
    ("id_u32_max_stays", [([5, 0xFFFFFFFF, 9], [6, 0xFFFFFFFE, 7])], [0xFFFFFFFE, 5], 4),
    ("ids_in_no_tree", [(A, B), [40, 50]], [0, 7, 39, 41, 51, 1000], 4),
    ("nothing_listed", [(A, B), (A + [9], B)], [], 4),
    ("nothing_listed_siblings_fit", [(A, [4])], [], 4),
    ("everything", [(A, B), (([20, 21], [22, 23]), [24]), [30, 31]], A + B + [20, 21, 22, 23, 24, 30, 31], 4),
    # a merged segment and a root list past what one block sorts in LDS (4096 ids): sorted in place in device memory
    ("merge_past_lds_sort", [(list(range(0, 6000, 2)), list(range(1, 5001, 2)))], list(range(0, 6000, 20)), 6000),
    ("roots_past_lds_sort", [([10000 + 2 * t], [10001 + 2 * t]) for t in range(50)] + [[t] for t in range(4100)],
     [10000 + 2 * t for t in range(50)], 1),
    ("many_rules_at_once", [(A, B), ((([1, 9], [2, 10]), [3, 11]), [4, 12]), CHAIN, SIZES, [77]], [1, 2, 3, 9, 10, 11, 12, 77, 1000, 5000]
     + [100 + 3 * d for d in range(75)], 5),
]


@pytest.mark.parametrize("name,specs,ids,split_after", HAND, ids=[h[0] for h in HAND])
def test_hand_made_views(small, name, specs, ids, split_after):
    store = make_store(specs)
    want = check(small, store, ids, split_after)
    if name == "both_empty_right_survives":
        assert len(want.nodes) == 1 and want.nodes[want.roots[0]][1].size == 0 and want.roots[0] == max(store.nodes)
    if name == "root_replaced_order_changes":
        assert want.roots != [r for r in store.roots] and want.roots[0] == store.roots[1]
    if name == "cascade_three_levels":
        assert len(want.nodes) == 1 and want.nodes[want.roots[0]][1].tolist() == [1, 2, 3, 4]
    if name == "one_more_stays_split":
        assert want.nodes[want.roots[0]][0] == "S"


# ---- 2. random forests -----------------------------------------------------------------------------------------------------

N = 20_000
WORLD_IDS = np.arange(N, dtype=np.uint32) * 3 + 7   # sparse ids


class World:
    def __init__(self, dist, split_after):
        self.dist, self.split_after = dist, split_after
        self.vecs = O.synth(21, 1, N, DIMS)
        self.ds = Dataset(dist, DIMS, N)
        self.ds.upload_vectors(WORLD_IDS, self.vecs)
        self.ds.finalize()
        self.seeds = [11, 12, 13]
        forest = self.ds.build_forest(self.seeds, split_after=split_after)
        self.store = TreeStore()
        self.store.roots = [self.store.next_id() for _ in self.seeds]
        for t, root in enumerate(self.store.roots):
            self.store.import_tree(forest, t, root_id=root)
        forest.close()
        g = np.random.default_rng(split_after)
        self.perm = g.permutation(WORLD_IDS)
        self.queries = self.vecs[g.integers(0, N, 64)] + np.float32(1e-3)
        self.route = np.sort(g.choice(WORLD_IDS, 500, replace=False)).astype(np.uint32)
        self.cand = np.sort(g.choice(WORLD_IDS, N // 3, replace=False)).astype(np.uint32)

    def deleted(self, share):
        return np.sort(self.perm[:int(round(N * share))])

    def close(self):
        self.ds.close()


@pytest.fixture(scope="module", params=[("Euclidean", 1), ("Euclidean", 8), ("Euclidean", 64), ("BinaryQuantizedEuclidean", 8)],
                ids=lambda p: f"{p[0]}-{p[1]}")
def world(request):
    w = World(getattr(D, request.param[0]), request.param[1])
    yield w
    _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
    w.close()


def same_answers(w, ix, dense, want_store, search=True, nonempty=True):
    """searches and routings of the updated index `ix` against a fresh index of the store after the delete"""
    view, keep = want_store.to_view(w.dist, DIMS)
    fresh = Index(w.ds, None, view=view)
    try:
        back_old = {i: nid for nid, i in dense.items()}
        back_new = {i: nid for nid, i in keep[4].items()}
        a, b = ix.route_items(w.route, w.seeds), fresh.route_items(w.route, w.seeds)
        assert a.shape == b.shape == (3, 500)
        assert [back_old[int(x)] for x in a.ravel()] == [back_new[int(x)] for x in b.ravel()]
        if search:
            for cand in (None, w.cand):
                x = ix.search(10, queries=w.queries, search_k=500, candidates=cand, candidates_sorted=True, raw=True)
                y = fresh.search(10, queries=w.queries, search_k=500, candidates=cand, candidates_sorted=True, raw=True)
                assert np.array_equal(x[2], y[2]) and np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes()
                if nonempty:
                    assert cand is not None or int(x[2].min()) > 0
                else:
                    assert not x[2].any() and not y[2].any()
    finally:
        fresh.close()


@pytest.mark.parametrize("share", [0.01, 0.30, 0.90, 1.0])
def test_random_forest(world, share):
    w = world
    if w.split_after <= 8:
        assert len(w.store.nodes) > 2 * 4096  # the scans over the nodes are past one tile (4096 words)
    ids = w.deleted(share)
    got, ix, dense = device_delete(w.ds, w.store, ids, w.split_after, w.dist)
    try:
        want = host_delete(w.store, ids, w.split_after)
        same_store(got, want)
        # (with every id gone the trees are three empty roots: both indexes answer every query with nothing)
        same_answers(w, ix, dense, want, nonempty=share < 1.0)
    finally:
        ix.close()


def test_random_forest_in_several_launches(world):
    """AH_LAUNCH_MAX_ITEMS cuts the count and write passes into launches of that many nodes"""
    w = world
    ids = w.deleted(0.30)
    with _lib.tuning(AH_LAUNCH_MAX_ITEMS=1000):
        got, ix, dense = device_delete(w.ds, w.store, ids, w.split_after, w.dist)
    try:
        want = host_delete(w.store, ids, w.split_after)
        same_store(got, want)
        same_answers(w, ix, dense, want, search=w.split_after == 8)
    finally:
        ix.close()


def test_two_deletes_chained_on_one_index(world):
    w = world
    first, second = w.deleted(0.30), np.sort(w.perm[int(N * 0.25):int(N * 0.70)])
    got, ix, dense = device_delete(w.ds, w.store, first, w.split_after, w.dist)
    try:
        got.apply_delta(ix.delete_items(second, w.split_after), dense)
        want = host_delete(host_delete(w.store, first, w.split_after), second, w.split_after)
        same_store(got, want)
        same_answers(w, ix, dense, want, search=w.split_after != 1)
    finally:
        ix.close()


# ---- 3. the state around it ------------------------------------------------------------------------------------------------

def refused(fn, text):
    with pytest.raises(_lib.ArroyHipError) as e:
        fn()
    assert e.value.status == 5 and text in e.value.message, e.value.message


def test_live_filter_refuses(world):
    w = world
    ids = w.deleted(0.01)
    view, keep = w.store.to_view(w.dist, DIMS)
    ix = Index(w.ds, None, view=view)
    try:
        f = ix.make_filter(w.cand, sorted=True)
        refused(lambda: ix.delete_items(ids, w.split_after), "live filters")
        assert _lib.lib().ah_index_suspend(ix._h) == 5 and b"live filters" in _lib.lib().ah_last_error()
        f.close()
        got = clone(w.store)
        got.apply_delta(ix.delete_items(ids, w.split_after), keep[4])
        same_store(got, host_delete(w.store, ids, w.split_after))
    finally:
        ix.close()


def test_suspend_update_resume():
    n = 4000
    vecs = O.synth(5, 1, n + 200, DIMS)
    ids = np.arange(n, dtype=np.uint32) * 2
    ds = Dataset(D.Euclidean, DIMS, n)
    ds.upload_vectors(ids, vecs[:n])
    ds.finalize()
    others = []
    try:
        forest = ds.build_forest([1, 2, 3], split_after=16)
        view = forest.view_struct()
        ix = Index(ds, None, view=view)
        queries = vecs[[3, 30, 300, 3000]] + np.float32(1e-3)
        changed = ids[100:300]
        refused(lambda: ds.update_vectors(np.zeros(0, np.uint32), changed, vecs[n:n + 200]), "alive")
        refused(lambda: ix.resume(), "not suspended")
        ix.suspend()
        refused(lambda: ix.suspend(), "suspended")
        refused(lambda: ix.search(5, queries=queries), "suspended")
        refused(lambda: ix.search(5, queries=queries, filters=[], filter_of_query=None), "suspended")
        refused(lambda: ix.route_items(ids[:5], [1, 2, 3]), "suspended")
        refused(lambda: ix.delete_items(ids[:5], 16), "suspended")
        refused(lambda: ix.make_filter(ids[:5], sorted=True), "suspended")
        ds.update_vectors(np.zeros(0, np.uint32), changed, vecs[n:n + 200])  # the same ids, other vectors: rows rewritten
        # resume: only on the dataset the index was made on, finalized
        for metric, dims, text in ((D.Euclidean, DIMS, "not the one"), (D.Cosine, DIMS, "metric"), (D.Euclidean, 32, "dimensions")):
            other = Dataset(metric, dims, 10)
            others.append(other)
            other.upload_vectors(np.arange(10, dtype=np.uint32), O.synth(1, 1, 10, dims))
            if text == "not the one":
                with pytest.raises(_lib.ArroyHipError) as e:
                    ix.resume(other)
                assert e.value.status == 7  # not finalized
            other.finalize()
            refused(lambda: ix.resume(other), text)
        import arroy_amd
        if arroy_amd.device_count() > 1:
            other = Dataset(D.Euclidean, DIMS, 10, device=1)
            others.append(other)
            other.upload_vectors(np.arange(10, dtype=np.uint32), O.synth(1, 1, 10, DIMS))
            other.finalize()
            refused(lambda: ix.resume(other), "device")
        ix.resume()
        fresh = Index(ds, None, view=view)
        for kw in (dict(queries=queries), dict(items=changed[:4])):
            a, b = ix.search(10, search_k=400, raw=True, **kw), fresh.search(10, search_k=400, raw=True, **kw)
            assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
        assert np.array_equal(ix.route_items(changed[:50], [1, 2, 3]), fresh.route_items(changed[:50], [1, 2, 3]))
        fresh.close()
        # a suspended index that is destroyed leaves no hold behind
        ix.suspend()
        ix.close()
        ds.update_vectors(ids[:10], np.zeros(0, np.uint32), np.zeros((0, DIMS), np.float32))
        assert len(ds) == n - 10
        forest.close()
    finally:
        for o in others:
            o.close()
        ds.close()


# ---- 4. allocation faults -------------------------------------------------------------------------------------------------

def test_delete_survives_every_allocation_failure(world):
    """AH_FAIL_ALLOC_AFTER = 1, 2, ... (tests/test_gpu_faults.py): every allocation of the call fails once; the call returns a
    status, holds no memory afterwards, and the index answers exactly as before; without the fault the call succeeds."""
    w = world
    ids = w.deleted(0.30)
    view, keep = w.store.to_view(w.dist, DIMS)
    ix = Index(w.ds, None, view=view)
    try:
        q = w.queries[:8]
        before = (ix.search(10, queries=q, search_k=500, raw=True), ix.route_items(w.route, w.seeds))
        seen = []
        for n in range(1, 200):
            live0, _ = _lib.device_cache_stats(0)
            _lib.tuning_set("AH_FAIL_ALLOC_AFTER", n)
            try:
                delta, status = ix.delete_items(ids, w.split_after), OK
            except _lib.ArroyHipError as e:
                delta, status = None, e.status
            finally:
                left = _lib.tuning_get("AH_FAIL_ALLOC_AFTER")[0]
                _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
            if left > 0:  # the counter never fired: every allocation of the call has failed once
                assert status == OK
                break
            assert status in (OOM, DEVICE), (n, status)
            assert _lib.lib().ah_last_error() != b""
            assert _lib.device_cache_stats(0)[0] <= live0, n
            now = (ix.search(10, queries=q, search_k=500, raw=True), ix.route_items(w.route, w.seeds))
            assert np.array_equal(now[0][0], before[0][0]) and now[0][1].tobytes() == before[0][1].tobytes(), n
            assert np.array_equal(now[0][2], before[0][2]) and np.array_equal(now[1], before[1]), n
            seen.append(status)
        else:
            raise AssertionError("more than 200 allocations in one call?")
        assert len(seen) >= 7 and OOM in seen, seen  # the bitmap, the work block, nodes, roots, ranks, blob, delta + host vectors
        got = clone(w.store)
        got.apply_delta(delta, keep[4])
        want = host_delete(w.store, ids, w.split_after)
        same_store(got, want)
        same_answers(w, ix, keep[4], want, search=w.split_after == 8)
    finally:
        ix.close()


# ---- 5. Writer -------------------------------------------------------------------------------------------------------------

def run_writer(dist, device_delete_on):
    dims, n0 = 24, 900
    g = np.random.default_rng(5)
    vecs = g.standard_normal((n0 + 700, dims)).astype(np.float32)
    db = I.Database(dist)
    w = I.Writer(db, 0, dims)
    st = w._st
    snaps = []

    def build(k, n_trees=5):
        b = w.builder(random.Random(40 + k)).n_trees(n_trees)
        b.device_delete = device_delete_on
        b.build()
        reader = I.Reader.open(db, 0)
        qs = vecs[[1, 500, 950, 1300]]
        snaps.append((clone(st.trees), copy.deepcopy(st.metadata), [reader.nns(10).search_k(300).by_vector(q) for q in qs],
                      reader.nns(5).by_item(st.metadata["items"][3]), st.device_deletes))
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
    for i in range(n0 + 300, n0 + 330):  # a build that drops two trees
        w.add_item(i, vecs[i])
    build(4, n_trees=3)
    for i in range(500, 520):
        assert w.del_item(i)
    build(5, n_trees=3)
    if st.index is not None:
        st.index.close()
    if st.dataset is not None:
        st.dataset.close()
    return snaps


@pytest.mark.parametrize("dist_name", ["Euclidean", "BinaryQuantizedCosine"])
def test_writer_takes_the_device_path_and_builds_the_same_trees(dist_name):
    dist = getattr(D, dist_name)
    dev, host = run_writer(dist, True), run_writer(dist, False)
    assert [s[4] for s in host] == [0] * 6
    # builds 1 - 3 and 5 are incremental on the updated dataset and drop no tree; build 4 drops two
    assert [s[4] for s in dev] == [0, 1, 2, 3, 3, 4]
    for k, (a, b) in enumerate(zip(dev, host)):
        same_store(a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3], k
        assert len(a[0].roots) == (5 if k < 4 else 3)


def test_writer_build_closes_a_reader_filter_that_is_still_alive():
    """A Filter of `Reader.make_filter` is "closed with its index at the latest": an incremental build that keeps the index for
    its delete and routing closes the filter before it suspends the index, as the host path does by closing the index."""
    dims, n0 = 24, 900
    vecs = np.random.default_rng(7).standard_normal((n0 + 100, dims)).astype(np.float32)
    db = I.Database(D.Euclidean)
    w = I.Writer(db, 0, dims)
    for i in range(n0):
        w.add_item(i, vecs[i])
    w.builder(random.Random(1)).n_trees(4).build()
    reader = I.Reader.open(db, 0)
    f = reader.make_filter(range(0, n0, 2))
    assert all(i % 2 == 0 for i, _ in reader.nns(5).candidates(f).by_vector(vecs[3]))
    for i in range(n0, n0 + 100):
        w.add_item(i, vecs[i])
    for i in range(0, 40):
        assert w.del_item(i)
    w.builder(random.Random(2)).n_trees(4).build()
    st = w._st
    assert st.device_deletes == 1 and not f._h
    reader = I.Reader.open(db, 0)
    f2 = reader.make_filter(range(0, n0 + 100, 2))
    got = reader.nns(5).candidates(f2).by_vector(vecs[3])
    assert len(got) == 5 and all(i % 2 == 0 and i >= 40 for i, _ in got)
    f2.close()
    st.index.close()
    st.dataset.close()
