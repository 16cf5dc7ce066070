"""Resident forests (include/arroy_hip.h, "Resident forests"): ah_build_forest_resident / ah_build_subtrees_resident keep the
arrays an index holds of the forest on the device, ah_index_create_from_forest / ah_index_graft_forest read them there.  The
yardsticks are the calls they stand in for: the digest of ah_build_forest with the same seeds, the export of ah_index_create,
the index ah_index_create_from_view makes of the store listed in ascending id order (TreeStore.import_tree + to_view), and
ah_index_graft of the same view on a twin index — bit for bit, searches and routings included.  Shapes: n = 3000 rows and
split_after = 16 (deep trees, several hundred nodes per tree), every metric, dims on either side of the `dims >= 32` paths, a
BQ width that is no multiple of 64, three batches, the grouped tail, several launch spans, trees that are one Descendants root."""
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

from test_gpu_faults import sweep_once  # noqa: E402
from test_gpu_index_delete import clone, same_store  # noqa: E402
from test_gpu_index_insert import DIMS as DIMS64, host_cycle, index_of, index_of_map, same_index  # noqa: E402

N, SPLIT = 3000, 16
NONE = 0xFFFFFFFF
OK, DEVICE, OOM = 0, 3, 4
SEEDS = [11, 12, 13, 14, 15]
IDS = np.arange(N, dtype=np.uint32) * 3 + 7  # sparse ids: rows and ids differ


class World:
    def __init__(self, dist, dims, clustered=False, n=N):
        import arroy_amd
        assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
        self.dist, self.dims, self.n = dist, dims, n
        self.ids = IDS[:n]
        self.vecs = O.synth(31, O.SYNTH_CLUSTERED if clustered else O.SYNTH_UNIFORM_PM1, n, dims)
        if clustered:  # runs of exact duplicates longer than split_after: their nodes find no plane (`normal: None`)
            for first, count in ((100, 40), (1000, 70), (2000, 20)):
                self.vecs[first:first + count] = self.vecs[first]
        self.ds = ds = Dataset(dist, dims, n)
        ds.upload_vectors(self.ids, self.vecs)
        if dist.metric == 3:
            ds.preprocess_dot()
        ds.finalize()
        g = np.random.default_rng(dims)
        self.queries = self.vecs[g.integers(0, n, 6)] + np.float32(1e-3)
        self.items = self.ids[g.integers(0, n, 6)]
        self.cand = np.sort(g.choice(self.ids, n // 3, replace=False)).astype(np.uint32)

    def close(self):
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        self.ds.close()


CASES = [("Euclidean", 40, False), ("Manhattan", 40, False), ("Cosine", 40, False), ("DotProduct", 40, False),
         ("BinaryQuantizedEuclidean", 40, False), ("BinaryQuantizedManhattan", 70, False), ("BinaryQuantizedCosine", 40, False),
         ("Euclidean", 24, False), ("Cosine", 24, False), ("Euclidean", 40, True)]


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"{p[0]}-{p[1]}" + ("-clustered" if p[2] else ""))
def world(request):
    w = World(getattr(D, request.param[0]), request.param[1], request.param[2])
    w.clustered = request.param[2]
    yield w
    w.close()


@pytest.fixture(scope="module", params=[("Euclidean", 40), ("BinaryQuantizedManhattan", 70)], ids=lambda p: f"{p[0]}-{p[1]}")
def world2(request):
    w = World(getattr(D, request.param[0]), request.param[1])
    yield w
    w.close()


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def export_bytes(ix):
    e = ix.export()
    return {k: np.ascontiguousarray(v).tobytes() for k, v in e.items()}


def answers(w, ix, n_trees):
    """every search the issue names, raw, and the routing of every item"""
    out = []
    for cand in (None, w.cand):
        out.append(ix.search(10, queries=w.queries, search_k=200, candidates=cand, candidates_sorted=True, raw=True))
        out.append(ix.search(10, items=w.items, search_k=200, candidates=cand, candidates_sorted=True, raw=True))
    flat = [np.ascontiguousarray(a).tobytes() for res in out for a in res]
    return flat + [ix.route_items(w.ids, SEEDS[:n_trees]).tobytes()]


def store_of(forest):
    """the host's store of a full build: the roots first, then every tree's nodes children before parents; -> (store, new_index)"""
    store = TreeStore()
    store.roots = [store.next_id() for _ in range(forest.n_trees)]
    maps = []
    for t, root in enumerate(store.roots):
        store.import_tree(forest, t, root_id=root)
        maps.append(store.last_import)
    dense = {nid: i for i, nid in enumerate(sorted(store.nodes))}
    new_index = np.full(len(forest.nodes), NONE, dtype=np.uint32)
    for ids_of in maps:
        for k, nid in ids_of.items():
            new_index[k] = dense[nid]
    assert sorted(new_index.tolist()) == list(range(len(forest.nodes)))
    return store, new_index


def same_as_fresh(w, ix, fresh):
    """`ix` (the store's numbering, made by a graft) against the index of the store's view: nodes, roots, every node's list and
    the row every split node resolves to; then both compacted, byte for byte."""
    a, b = ix.export(), fresh.export()
    assert np.array_equal(a["roots"], b["roots"])
    for f in ("kind", "has_normal", "left", "right", "count"):
        assert np.array_equal(a["nodes"][f], b["nodes"][f]), f
    for x, y in zip(a["nodes"], b["nodes"]):
        if x["kind"] == 1:
            assert np.array_equal(a["descendants"][int(x["offset"]):int(x["offset"]) + int(x["count"])],
                                  b["descendants"][int(y["offset"]):int(y["offset"]) + int(y["count"])])
        elif x["has_normal"]:
            assert a["normal_rows"][int(x["offset"])].tobytes() == b["normal_rows"][int(y["offset"])].tobytes()
            assert a["normal_headers"][int(x["offset"])].tobytes() == b["normal_headers"][int(y["offset"])].tobytes()
    n_trees = len(a["roots"])
    assert answers(w, ix, n_trees) == answers(w, fresh, n_trees)
    ix.compact()
    fresh.compact()
    assert export_bytes(ix) == export_bytes(fresh)


def check_forest(w, n_trees=5, split_after=SPLIT, oracle=False, **kw):
    """Every equality of one shape case.  -> the stats of the resident build"""
    ds, seeds = w.ds, SEEDS[:n_trees]
    plain = ds.build_forest(seeds, split_after=split_after, **kw)
    res = ds.build_forest(seeds, split_after=split_after, resident=True, **kw)
    res2 = ds.build_forest(seeds, split_after=split_after, resident=True, **kw)
    res3 = ds.build_forest(seeds, split_after=split_after, resident=True, **kw)
    made = []
    try:
        assert not plain.resident and plain.device_bytes == 0
        assert res.resident and res.device_bytes >= 4 * res.descendants.size
        assert res.digest()[0] == plain.digest()[0] and np.array_equal(res.digest()[1], plain.digest()[1])
        # the forest's own numbering: the index of ah_index_create, on the forest's blocks
        a = Index(ds, plain)
        b = Index.from_forest(ds, res)
        made += [a, b]
        assert b.from_device and not res.resident and res.device_bytes == 0
        want = export_bytes(a)
        assert export_bytes(b) == want
        c = Index.from_forest(ds, res)  # consumed: the host view, the same index
        made.append(c)
        assert not c.from_device and export_bytes(c) == want
        ref = answers(w, a, n_trees)
        assert answers(w, b, n_trees) == ref
        if oracle:
            od = O.Data(w.dist.metric, w.vecs, ids=w.ids)
            got = b.search(10, queries=w.queries, search_k=200)
            for i, q in enumerate(w.queries):
                v, h = od.query_leaf(q)
                exp, _ = O.search(od, plain, v, h, 10, 200)
                assert [x for x, _ in got[i]] == [x for x, _ in exp]
                assert np.array([y for _, y in got[i]], np.float32).tobytes() == np.array([y for _, y in exp], np.float32).tobytes()
        # the store's numbering
        store, new_index = store_of(plain)
        view, keep = store.to_view(w.dist, w.dims)
        fresh = Index(ds, None, view=view)
        d = Index.from_forest(ds, res2, new_index)
        made += [fresh, d]
        assert d.from_device and not res2.resident
        stats = dict(res2.stats)
        res2.close()  # the forest may go before the index is searched
        res3.release_device()
        assert not res3.resident
        e = Index.from_forest(ds, res3, new_index)  # released: the host view
        made.append(e)
        assert not e.from_device
        assert export_bytes(e)["nodes"] == export_bytes(d)["nodes"] and export_bytes(e)["descendants"] == export_bytes(d)["descendants"]
        same_as_fresh(w, d, fresh)
        e.compact()
        assert export_bytes(e) == export_bytes(d)
        return stats
    finally:
        for ix in made:
            ix.close()
        for f in (plain, res, res2, res3):
            f.close()


# ---- 1. full builds -----------------------------------------------------------------------------------------------------------

def test_three_batches_every_metric(world):
    """5 trees, two in flight: three batches; every row of the later batches lands behind the rows of the batches before"""
    w = world
    stats = check_forest(w, max_trees_in_flight=2, oracle=w.dist.metric != 3)
    assert stats["split_nodes"] > 5 * 100
    if w.clustered:  # exact duplicate rows: nodes whose two-means found no plane get no row
        assert stats["dummy_normals"] > 0


def test_grouped_tail(world2):
    with _lib.tuning(AH_BUILD_TAIL_GROUPS=3, AH_BUILD_TAIL_MIN_MB=0, AH_ROWMAJOR=0):
        stats = check_forest(world2)
    assert stats["tail_groups"] >= 2


def test_several_launch_spans(world2):
    with _lib.tuning(AH_LAUNCH_MAX_ITEMS=100):
        stats = check_forest(world2, n_trees=3)
    assert stats["split_nodes"] - stats["dummy_normals"] > 3 * 100  # the rows kernel ran in more than three spans


def test_every_tree_is_one_descendants_root():
    w = World(D.Euclidean, 40, n=12)
    try:
        stats = check_forest(w, n_trees=3)
        assert stats["split_nodes"] == 0 and stats["descendant_nodes"] == 3
    finally:
        w.close()


def test_another_dataset_takes_the_host_view(world2):
    """A forest resident for other dimensions than the dataset's: the call is ah_index_create of the same forest on that dataset
    — the same index, or the same refusal — and the device copy stays.  (Euclidean 40 -> 104 dimensions: the vector no longer
    fits the record, refused; 1-bit 70 -> 134 bits: 24 bytes fit the 32-byte record, accepted.)  The other fall-back the header
    names, a forest that lives on another device, needs two GPUs and is not tested here."""
    w = world2
    other = World(w.dist, w.dims, n=200)
    wrong = World(w.dist, w.dims + 64, n=200)
    g = other.ds.build_forest(SEEDS[:2], split_after=SPLIT, resident=True)

    def outcome(make):
        try:
            ix = make()
        except _lib.ArroyHipError as e:
            return ("refused", e.status)
        try:
            return ("made", export_bytes(ix), answers(wrong, ix, 2), getattr(ix, "from_device", False))
        finally:
            ix.close()
    try:
        want = outcome(lambda: Index(wrong.ds, g))
        assert want[0] == ("refused" if w.dist.metric < 4 else "made")
        for new_index in (None, np.arange(len(g.nodes), dtype=np.uint32)):
            got = outcome(lambda: Index.from_forest(wrong.ds, g, new_index))
            assert g.resident
            assert got[0] == want[0] and got[-1] == (want[1] if want[0] == "refused" else False)
            if want[0] == "made" and new_index is None:
                assert got[1] == want[1] and got[2] == want[2]
            elif want[0] == "made":  # (the identity renumbering, through the graft: the same answers)
                assert got[2] == want[2]
        ix = Index.from_forest(other.ds, g)  # ... and on its own dataset the copy still serves
        assert ix.from_device and not g.resident
        ix.close()
    finally:
        g.close()
        wrong.close()
        other.close()


def test_memory_returns_to_its_start():
    live0, _ = _lib.device_cache_stats(0)
    w = World(D.Cosine, 40)
    f = w.ds.build_forest(SEEDS[:3], split_after=SPLIT, resident=True)
    g = w.ds.build_forest(SEEDS[:3], split_after=SPLIT, resident=True)
    ix = Index.from_forest(w.ds, f)
    assert ix.from_device
    f.close()
    got = ix.search(5, queries=w.queries, search_k=100, raw=True)
    assert got[2].min() == 5
    g.close()  # a resident forest nobody consumed
    ix.close()
    w.close()
    assert _lib.device_cache_stats(0)[0] == live0


# ---- 2. sub-trees and grafts -----------------------------------------------------------------------------------------------------

class SubWorld:
    """the world of tests/test_gpu_index_insert.py at 3000 rows: three trees, half of the items in no tree yet"""
    def __init__(self, dist, split_after):
        from test_gpu_index_delete import host_delete
        self.dist, self.split_after = dist, split_after
        self.vecs = O.synth(21, 1, N, DIMS64)
        self.ds = ds = Dataset(dist, DIMS64, N)
        ds.upload_vectors(IDS, self.vecs)
        ds.finalize()
        self.seeds = [11, 12, 13]
        forest = ds.build_forest(self.seeds, split_after=split_after)
        self.store = TreeStore()
        self.store.roots = [self.store.next_id() for _ in self.seeds]
        for t, root in enumerate(self.store.roots):
            self.store.import_tree(forest, t, root_id=root)
        forest.close()
        g = np.random.default_rng(split_after)
        self.perm = g.permutation(IDS)
        self.store = host_delete(self.store, self.perm[N // 2:], split_after)
        ds.queries = self.vecs[g.integers(0, N, 16)] + np.float32(1e-3)
        ds.route_ids = IDS
        ds.cand = np.sort(g.choice(IDS, N // 3, replace=False)).astype(np.uint32)

    def updated(self, share, first=0):
        half = int(round(N * share)) // 2
        return np.sort(np.concatenate([self.perm[first:first + half], self.perm[N // 2 + first:N // 2 + first + half]]))


@pytest.fixture(scope="module", params=["Euclidean", "BinaryQuantizedEuclidean"])
def sub(request):
    w = SubWorld(getattr(D, request.param), SPLIT)
    yield w
    _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
    w.ds.close()


def subtree_round(w, store, ids, round_seed, extra_small=False):
    """One incremental build on the host: -> (mid, end, the re-split nodes, their id lists, seeds, maps of a plain build, its forest)"""
    mid, _end, large, f0, _maps = host_cycle(w, store, ids, round_seed)
    if f0 is not None:
        f0.close()
    assert large, "no node outgrew split_after"
    nids = list(large)
    if extra_small:  # a list that fits a single node: its tree is one Descendants root, which replaces the node by itself
        nids.append(next(nid for nid in sorted(mid.nodes) if mid.nodes[nid][0] == "D" and nid not in large
                         and 0 < len(mid.nodes[nid][1]) <= w.split_after))
    lists = [mid.nodes[nid][1] for nid in nids]
    seeds = [round_seed + t for t in range(len(nids))]
    plain = w.ds.build_subtrees(lists, seeds, w.split_after)
    end = clone(mid)
    end._next, end._available = mid._next, list(mid._available)
    maps = []
    for t, nid in enumerate(nids):
        end.import_tree(plain, t, root_id=nid)
        maps.append(end.last_import)
    return mid, end, nids, lists, seeds, maps, plain


def graft_args(end, nids, maps, forest, dense):
    new_dense = index_of_map(end)
    new_index = np.full(len(forest.nodes), NONE, dtype=np.uint32)
    for t, ids_of in enumerate(maps):
        for k, nid in ids_of.items():
            new_index[k] = new_dense[nid]
        new_index[int(forest.roots[t])] = NONE
    return new_dense, np.array([dense[nid] for nid in nids], dtype=np.uint32), new_index


def test_subtrees_graft_like_the_view_on_a_twin(sub):
    w = sub
    # (the second update brings in every item that is in no tree yet: afterwards the index holds each item once per tree)
    ids1, ids2 = w.updated(0.2), np.sort(np.concatenate([w.perm[N // 8:N // 8 + 300], w.perm[N // 2:]]))
    r1 = subtree_round(w, w.store, ids1, 100, extra_small=True)
    r2 = subtree_round(w, r1[1], ids2, 200)
    twin, dense = index_of(w.ds, w.store, w.dist)
    mine, _ = index_of(w.ds, w.store, w.dist)
    forests = [r1[6], r2[6]]
    try:
        store = w.store
        for k, (mid, end, nids, lists, seeds, maps, plain) in enumerate((r1, r2)):
            res = w.ds.build_subtrees(lists, seeds, w.split_after, resident=True)
            forests.append(res)
            assert res.resident and res.digest()[0] == plain.digest()[0]
            if k == 0:
                assert any(plain.nodes[int(plain.roots[t])]["kind"] == 1 for t in range(plain.n_trees))
            for ix in (twin, mine):
                got = clone(store)
                got.apply_delta(ix.delete_items(ids1 if k == 0 else ids2, w.split_after), dense)
                got.apply_delta(ix.insert_items(ids1 if k == 0 else ids2, w.seeds), dense)
                same_store(got, mid)
            new_dense, targets, new_index = graft_args(end, nids, maps, plain, dense)
            map_a = twin.graft(plain.view_struct(), targets, new_index, want_map=True)
            from_device, map_b = mine.graft_forest(res, targets, new_index, want_map=True)
            assert from_device and not res.resident and np.array_equal(map_a, map_b)
            assert export_bytes(mine) == export_bytes(twin)
            dense, store = new_dense, end
        same_index(w.ds, mine, dense, store, w.seeds, w.dist, strict=True)
        for ix in (twin, mine):
            ix.compact()
        assert export_bytes(mine) == export_bytes(twin)
        ra, rb = mine.audit(trees=True), twin.audit(trees=True)
        from arroy_amd.dataset import audit_findings
        assert ra["valid"], audit_findings(ra)
        assert ra == rb
        # a consumed forest grafts through its host view: refused here only because its targets are gone
        with pytest.raises(_lib.ArroyHipError):
            mine.graft_forest(forests[-1], np.full(forests[-1].n_trees, 10 ** 9, dtype=np.uint32), None)
    finally:
        twin.close()
        mine.close()
        for f in forests:
            f.close()


def test_graft_forest_refusals_leave_forest_and_index_as_they_were(sub):
    w = sub
    mid, end, nids, lists, seeds, maps, plain = subtree_round(w, w.store, w.updated(0.2), 100)
    ix, dense = index_of(w.ds, w.store, w.dist)
    res = w.ds.build_subtrees(lists, seeds, w.split_after, resident=True)
    try:
        ix.delete_items(w.updated(0.2), w.split_after)
        ix.insert_items(w.updated(0.2), w.seeds)
        before = export_bytes(ix)
        new_dense, targets, new_index = graft_args(end, nids, maps, plain, dense)
        twice = targets.copy()
        twice[-1] = twice[0] if len(twice) > 1 else NONE - 1
        bad_index = new_index.copy()
        bad_index[np.flatnonzero(bad_index != NONE)[:2]] = 0
        for tg, ni in ((twice, new_index), (targets, bad_index)):
            with pytest.raises(_lib.ArroyHipError):
                ix.graft_forest(res, tg, ni)
            assert res.resident and export_bytes(ix) == before
        f = ix.make_filter(IDS[::2], sorted=True)
        with pytest.raises(_lib.ArroyHipError):
            ix.graft_forest(res, targets, new_index)
        f.close()
        assert res.resident and ix.graft_forest(res, targets, new_index)
        same_index(w.ds, ix, new_dense, end, w.seeds, w.dist, strict=True, search=False)
    finally:
        ix.close()
        res.close()
        plain.close()


# ---- 3. allocation faults ------------------------------------------------------------------------------------------------------

def test_resident_build_survives_every_allocation_failure(world2):
    w = world2
    seeds = SEEDS[:2]
    plain = w.ds.build_forest(seeds, split_after=64)
    want = plain.digest()[0]
    plain.close()
    kinds = set()

    def cleanup(f):
        assert f.digest()[0] == want
        kinds.add(f.resident)
        f.close()
    seen = sweep_once(lambda: w.ds.build_forest(seeds, split_after=64, resident=True), cleanup, 3000)
    assert OOM in seen and kinds == {True, False}  # (the device copy's own allocations fail into an ordinary forest)


def test_create_and_graft_from_a_forest_survive_every_allocation_failure(sub):
    w = sub
    mid, end, nids, lists, seeds, maps, plain = subtree_round(w, w.store, w.updated(0.2), 100)
    ix, dense = index_of(w.ds, w.store, w.dist)
    twin, _ = index_of(w.ds, w.store, w.dist)
    full = w.ds.build_forest(w.seeds, split_after=w.split_after)
    store, store_index = store_of(full)
    try:
        # create: AH_OK with the right index, or an error and no index (the forest stays resident for the next try)
        a = Index(w.ds, full)
        want = export_bytes(a)
        a.close()
        for new_index in (None, store_index):
            res = w.ds.build_forest(w.seeds, split_after=w.split_after, resident=True)
            outcomes = []

            def create():
                assert res.resident
                return Index.from_forest(w.ds, res, new_index)

            def created(made):
                outcomes.append(made.from_device)
                if new_index is None:
                    assert export_bytes(made) == want
                else:
                    view, keep = store.to_view(w.dist, DIMS64)
                    fresh = Index(w.ds, None, view=view)
                    made.compact()
                    fresh.compact()
                    assert export_bytes(made) == export_bytes(fresh)
                    fresh.close()
                made.close()
            seen = sweep_once(create, created, 400)
            assert outcomes == [True] and len(seen) >= 2 and OOM in seen
            res.close()
        # graft: AH_OK with the right index, or an error that leaves it unchanged and searchable
        for one in (ix, twin):
            one.delete_items(w.updated(0.2), w.split_after)
            one.insert_items(w.updated(0.2), w.seeds)
        new_dense, targets, new_index = graft_args(end, nids, maps, plain, dense)
        res = w.ds.build_subtrees(lists, seeds, w.split_after, resident=True)
        before = export_bytes(ix)
        q = w.ds.queries[:4]
        ref = [x.tobytes() for x in ix.search(10, queries=q, search_k=300, raw=True)]
        seen = []
        for n in range(1, 400):
            _lib.tuning_set("AH_FAIL_ALLOC_AFTER", n)
            try:
                from_device, status = ix.graft_forest(res, targets, new_index), OK
            except _lib.ArroyHipError as e:
                from_device, status = None, e.status
            finally:
                left = _lib.tuning_get("AH_FAIL_ALLOC_AFTER")[0]
                _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
            if status == OK:
                assert from_device and not res.resident
                break
            assert status in (DEVICE, OOM) and left == 0 and res.resident
            assert export_bytes(ix) == before
            assert [x.tobytes() for x in ix.search(10, queries=q, search_k=300, raw=True)] == ref
            seen.append(status)
        else:
            raise AssertionError("more than 400 allocations in one graft?")
        assert len(seen) >= 3 and OOM in seen
        twin.graft(plain.view_struct(), targets, new_index)
        assert export_bytes(ix) == export_bytes(twin)
        res.close()
    finally:
        ix.close()
        twin.close()
        full.close()
        plain.close()


# ---- 4. Writer ----------------------------------------------------------------------------------------------------------------

def run_writer(dist, device_forest):
    """the incremental sequence of tests/test_gpu_index_insert.py (run_writer): a full build, then adds, replacements and
    deletes, a build that adds trees, one that drops trees; every build keeps its index (device_insert)"""
    dims, n0 = 24, 900
    g = np.random.default_rng(5)
    vecs = g.standard_normal((n0 + 800, dims)).astype(np.float32)
    db = I.Database(dist)
    w = I.Writer(db, 0, dims)
    st = w._st
    snaps = []

    def build(k, n_trees=5):
        b = w.builder(random.Random(40 + k)).n_trees(n_trees)
        b.device_insert = True
        b.device_forest = device_forest
        b.build()
        reader = I.Reader.open(db, 0)
        qs = vecs[[1, 500, 950, 1300]]
        snaps.append((clone(st.trees), copy.deepcopy(st.metadata), [reader.nns(10).search_k(300).by_vector(q) for q in qs],
                      reader.nns(5).by_item(st.metadata["items"][3]), st.index_uploads))
    for i in range(n0):
        w.add_item(i, vecs[i])
    build(0)
    for i in range(n0, n0 + 300):
        w.add_item(i, vecs[i])
    for i in range(0, 50):
        w.add_item(i, vecs[n0 + 300 + i])
    for i in range(100, 200):
        assert w.del_item(i)
    build(1)
    for i in range(200, 400):
        assert w.del_item(i)
    build(2)
    for i in range(n0 + 300, n0 + 330):
        w.add_item(i, vecs[i])
    build(3, n_trees=7)
    view, keep = st.trees.to_view(dist, dims)
    fresh = Index(st.dataset, None, view=view)
    qs = vecs[[1, 500, 950, 1300]]
    a, b = st.index.search(10, queries=qs, search_k=300, raw=True), fresh.search(10, queries=qs, search_k=300, raw=True)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    fresh.close()
    st.index.close()
    st.dataset.close()
    return snaps


def play_reference_sequence(name, device_forest):
    """The item sequences of the reference's incremental snapshots that tests/test_gpu_reference_snapshots.py replays
    (src/tests/writer.rs:868-965 `add_one_item_incrementally`, :1123-1242 `reuse_node_id`: six points on a line, one tree, then
    one change per build), through ArroyBuilder.  The goldens themselves pin RefWriter, which draws the reference's own
    randomness; ArroyBuilder draws its tree seeds from a Python RNG, so here the yardstick is the same builder with the
    switch off."""
    from test_oracle_reference_incremental import line
    db = I.Database(D.Euclidean)
    w = I.Writer(db, 0, 2)
    st = w._st
    snaps = []

    def build(k, n_trees=1):
        b = w.builder(random.Random(7 + k)).n_trees(n_trees)
        b.device_insert = True
        b.device_forest = device_forest
        b.build()
        reader = I.Reader.open(db, 0)
        snaps.append((clone(st.trees), copy.deepcopy(st.metadata), reader.nns(3).by_vector(np.array([2.2, 0.0], np.float32)),
                      st.index_uploads))
    for i, v in line(6):
        w.add_item(i, np.array(v, np.float32))
    build(0)
    if name == "add_one_item_incrementally":
        w.add_item(25, np.array([25.0, 0.0], np.float32))
        build(1)
        w.add_item(8, np.array([8.0, 0.0], np.float32))
        build(2)
    else:
        assert w.del_item(4)
        build(1)
        w.add_item(4, np.array([4.0, 0.0], np.float32))
        build(2)
        build(3, n_trees=2)
    if st.index is not None:
        st.index.close()
    st.dataset.close()
    return snaps


@pytest.mark.parametrize("name", ["add_one_item_incrementally", "reuse_node_id"])
def test_reference_sequences_with_device_forest(name):
    on, off = play_reference_sequence(name, True), play_reference_sequence(name, False)
    assert [s[3] for s in on] == [0] * len(on) and off[0][3] == 1
    for k, (a, b) in enumerate(zip(on, off)):
        same_store(a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2], k


@pytest.mark.parametrize("dist_name", ["Euclidean", "BinaryQuantizedCosine"])
def test_writer_with_device_forest_builds_the_same_and_uploads_no_index(dist_name):
    dist = getattr(D, dist_name)
    on, off = run_writer(dist, True), run_writer(dist, False)
    assert [s[4] for s in off] == [1, 1, 1, 1]  # the first build uploads the index of its view, the others keep it
    assert [s[4] for s in on] == [0, 0, 0, 0]
    for k, (a, b) in enumerate(zip(on, off)):
        same_store(a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3], k
