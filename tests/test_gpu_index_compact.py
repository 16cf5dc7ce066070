"""ah_index_footprint_get and ah_index_compact (compaction of a resident index) and the Writer policy that uses them.  The
yardstick everywhere: after compact() the index must be, array for array, the index ah_index_create_from_view makes of the
host's store (`TreeStore.to_view`): nodes (a split node's `offset`, its normal ROW, included), roots, descendants, normal rows and
headers byte for byte, export_info and footprint (device_bytes included); the landing node of every dataset id in every tree
and the searches with and without candidates (ids, distance bits, counts) must agree as well."""
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
import test_gpu_index_insert as INS  # noqa: E402

NONE = 0xFFFFFFFF
INVALID = 5
SEEDS = [5, 6, 7, 8, 9, 10, 11, 12]
NODE_FIELDS = ("kind", "has_normal", "left", "right", "offset", "count")


class Ctx:
    """A dataset of n rows (ids 0 .. n - 1) with what the yardstick needs next to it."""

    def __init__(self, dist, dims, n, seed=3, queries=5, world=None):
        import arroy_amd
        assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
        self.dist, self.dims, self.n = dist, dims, n
        if world is not None:  # the dataset of a World of the insert tests
            self.ds, self.ids, self.queries, self.cand = world.ds, INS.WORLD_IDS, world.ds.queries, world.ds.cand
            return
        self.vecs = O.synth(seed, 1, n, dims)
        self.ids = np.arange(n, dtype=np.uint32)
        self.ds = Dataset(dist, dims, n)
        self.ds.upload_vectors(self.ids, self.vecs)
        if dist.metric == 3:
            self.ds.preprocess_dot()
        self.ds.finalize()
        g = np.random.default_rng(seed)
        self.queries = self.vecs[g.integers(0, n, queries)] + np.float32(1e-3)
        self.cand = np.sort(self.ids[::3])

    def close(self):
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        self.ds.close()

    def index_of(self, store):
        view, keep = store.to_view(self.dist, self.dims)
        return Index(self.ds, None, view=view), keep[4]


def make_store(ctx, specs, seed=1):
    """specs: one tree each; a list of ids is a Descendants node, a pair (left, right) a split node, every second one without a
    plane.  Roots get their ids first, then every tree its nodes, children before parents (as Writer does)."""
    g = np.random.default_rng(seed)
    s = TreeStore()
    hs, vs = ctx.dist.header_size(), ctx.dist.vector_size(ctx.dims)
    s.roots = [s.next_id() for _ in specs]
    planes = [0]

    def add(spec, nid=None):
        if isinstance(spec, tuple):
            left, right = add(spec[0]), add(spec[1])
            nid = s.next_id() if nid is None else nid
            planes[0] += 1
            if ctx.dist.name.startswith("binary"):
                vec = g.integers(0, 256, vs, dtype=np.uint8).tobytes()
            else:
                vec = g.standard_normal(vs // 4).astype(np.float32).tobytes()
            s.nodes[nid] = ("S", left, right, g.standard_normal(hs // 4).astype(np.float32), vec if planes[0] % 2 else None)
        else:
            nid = s.next_id() if nid is None else nid
            s.nodes[nid] = ("D", np.array(sorted(spec), dtype=np.uint32))
        return nid
    for root, spec in zip(s.roots, specs):
        add(spec, root)
    return s


def same_arrays(a, b):
    for f in NODE_FIELDS:
        assert np.array_equal(a["nodes"][f], b["nodes"][f]), f
    for key in ("roots", "descendants", "normal_rows", "normal_headers"):
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key


def exact(ctx, ix, store, seeds=SEEDS, search=True):
    """THE yardstick: `ix` against a fresh index of `store`, in every array and every answer."""
    fresh, _ = ctx.index_of(store)
    try:
        assert ix.export_info() == fresh.export_info()
        same_arrays(ix.export(), fresh.export())
        fa, fb = ix.footprint(), fresh.footprint()
        assert fa == fb, (fa, fb)
        assert fa["free_slots"] == 0 and fa["n_normals"] == fa["live_normals"] and fa["normals_cap"] == max(1, fa["n_normals"])
        n_trees = len(store.roots)
        if n_trees:
            sd = (seeds * (n_trees // len(seeds) + 1))[:n_trees]
            assert np.array_equal(ix.route_items(ctx.ids, sd), fresh.route_items(ctx.ids, sd))
        if search:
            for cand in (None, ctx.cand):
                for sk in (40, 10 ** 9):  # (the second opens every leaf)
                    x = ix.search(10, queries=ctx.queries, search_k=sk, candidates=cand, candidates_sorted=True, raw=True)
                    y = fresh.search(10, queries=ctx.queries, search_k=sk, candidates=cand, candidates_sorted=True, raw=True)
                    assert np.array_equal(x[2], y[2]) and np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes(), (sk, cand is None)
        return fa
    finally:
        fresh.close()


def check_map(before, m):
    """out_new_of_old: 0xFFFFFFFF exactly at the free slots of the export before the call, strictly increasing elsewhere"""
    free = before["nodes"]["kind"] == 0
    assert m.size == free.size and np.array_equal(m == NONE, free)
    used = m[~free].astype(np.int64)
    assert np.array_equal(used, np.arange(used.size))


def compact_and_check(ctx, ix, want, seeds=SEEDS, search=True):
    """compact, the map, the yardstick, and a second compaction that must find nothing to do"""
    before, fp0 = ix.export(), ix.footprint()
    stats, m = ix.compact(want_map=True)
    check_map(before, m)
    fp = exact(ctx, ix, want, seeds, search)
    assert stats["moved"] == 1
    assert (stats["nodes_before"], stats["normals_before"], stats["normals_cap_before"], stats["device_bytes_before"]) == (
        fp0["n_nodes"], fp0["n_normals"], fp0["normals_cap"], fp0["device_bytes"])
    assert (stats["nodes_after"], stats["normals_after"], stats["normals_cap_after"], stats["device_bytes_after"]) == (
        fp["n_nodes"], fp["n_normals"], fp["normals_cap"], fp["device_bytes"])
    assert stats["nodes_after"] == fp0["n_nodes"] - fp0["free_slots"] and stats["normals_after"] == fp0["live_normals"]
    live0 = _lib.device_cache_stats(0)[0]
    again, m2 = ix.compact(want_map=True)
    assert again["moved"] == 0 and np.array_equal(m2, np.arange(fp["n_nodes"])) and _lib.device_cache_stats(0)[0] == live0
    assert again["device_bytes_before"] == again["device_bytes_after"] == fp["device_bytes"]
    return before, m, stats


def delete_and_compact(ctx, store, ids, split_after, seeds=SEEDS, search=True):
    """delete `ids` on an index of `store`, compact it -> (the store afterwards, the export before the compaction, the map)"""
    ix, dense = ctx.index_of(store)
    try:
        got = clone(store)
        got.apply_delta(ix.delete_items(np.array(sorted(ids), dtype=np.uint32), split_after), dense)
        want = host_delete(store, ids, split_after)
        same_store(got, want)
        before, m, stats = compact_and_check(ctx, ix, want, seeds, search)
        assert [int(m[dense[nid]]) for nid in sorted(want.nodes)] == list(range(len(want.nodes)))
        return want, before, m, stats
    finally:
        ix.close()


# ---- 1. hand-made views, one per rule ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hand():
    ctx = Ctx(D.Euclidean, 32, 400)
    yield ctx
    ctx.close()


A, B = [1, 2, 3], [4, 5, 6]
TREE = (([11, 12, 13], [14, 15, 16]), ([17, 18], ([19, 20, 21], [22])))  # four split nodes
T = lambda k: ((list(range(k, k + 3)), list(range(k + 3, k + 6))), (list(range(k + 6, k + 9)), list(range(k + 9, k + 12))))  # noqa: E731
CHAIN = [100, 101, 102]
for _d in range(1, 75):  # 74 split levels, three ids a leaf
    CHAIN = ([100 + 3 * _d, 101 + 3 * _d, 102 + 3 * _d], CHAIN)


def test_an_index_without_a_split_node(hand):
    store = make_store(hand, [[1, 2, 3]])
    ix, dense = hand.index_of(store)
    try:
        fp = ix.footprint()
        assert (fp["n_nodes"], fp["free_slots"], fp["n_normals"], fp["live_normals"], fp["normals_cap"], fp["desc_len"]) == (1, 0, 0, 0, 1, 3)
        assert ix.compact()["moved"] == 0
        exact(hand, ix, store)
        ix.delete_items(np.array([2], dtype=np.uint32), 4)  # (no hole, but the delete leaves ranks)
        want = host_delete(store, [2], 4)
        before, m, stats = compact_and_check(hand, ix, want)
        assert stats["normals_cap_after"] == 1 and stats["normals_after"] == 0 and m.tolist() == [0]
        assert stats["device_bytes_after"] < stats["device_bytes_before"]
    finally:
        ix.close()


def test_nothing_to_do_allocates_nothing(hand):
    store = make_store(hand, [TREE, (A, B)])
    ix, dense = hand.index_of(store)
    try:
        live0 = _lib.device_cache_stats(0)[0]
        before = ix.export()
        stats, m = ix.compact(want_map=True)
        assert stats["moved"] == 0 and np.array_equal(m, np.arange(len(store.nodes)))
        assert stats["nodes_before"] == stats["nodes_after"] == len(store.nodes)
        assert stats["normals_before"] == stats["normals_after"] == stats["normals_cap_after"] == 3
        assert _lib.device_cache_stats(0)[0] == live0
        same_arrays(before, ix.export())
        exact(hand, ix, store)
        # an insert changes neither slots nor rows
        ix.insert_items(np.array([300, 301], dtype=np.uint32), SEEDS[:2])
        assert ix.compact()["moved"] == 0 and _lib.device_cache_stats(0)[0] == live0
    finally:
        ix.close()


def test_holes_at_the_first_a_middle_and_the_last_slot(hand):
    store = make_store(hand, [(A, B), TREE, (([30], [31]), [32, 33])])
    want, before, m, _ = delete_and_compact(hand, store, A + [17, 18] + [32, 33], 1)
    free = np.flatnonzero(before["nodes"]["kind"] == 0)
    assert free[0] == 0 and free[-1] == len(store.nodes) - 1 and any(0 < f < len(store.nodes) - 1 for f in free)
    assert any(nd[0] == "S" and nd[4] is None for nd in want.nodes.values())  # `normal: None` nodes among the live ones


def test_every_split_node_of_one_tree_removed(hand):
    store = make_store(hand, [T(40), T(60)])
    want, before, m, stats = delete_and_compact(hand, store, ids_of(T(40)), 4)
    kinds = sorted((want.nodes[r][0], len(want.nodes[r][1]) if want.nodes[r][0] == "D" else -1) for r in want.roots)
    assert kinds == [("D", 0), ("S", -1)]  # one tree is an empty Descendants root, the other keeps its rows
    assert stats["normals_before"] == 3 and stats["normals_after"] in (1, 2)


def test_dead_rows_in_front_of_between_and_behind_the_live_ones(hand):
    store = make_store(hand, [T(40), T(60), T(80), T(100), T(120)])
    want, before, m, stats = delete_and_compact(hand, store, ids_of(T(40)) + ids_of(T(80)) + ids_of(T(120)), 4)
    nd = before["nodes"]
    live = np.sort(nd["offset"][(nd["kind"] == 2) & (nd["has_normal"] == 1)].astype(np.int64))
    dead = np.setdiff1d(np.arange(stats["normals_before"]), live)
    assert dead.size and live.size and dead[0] < live[0] and dead[-1] > live[-1] and ((dead > live[0]) & (dead < live[-1])).any()
    assert stats["normals_after"] == live.size
    assert any(x[0] == "S" and x[4] is None for x in want.nodes.values())  # they own no row and do not shift the row ranks


def test_a_changed_root_order_survives(hand):
    store = make_store(hand, [(A, B), ([7, 8, 9], [10, 11, 12]), [20, 21]])
    want, before, m, _ = delete_and_compact(hand, store, A, 4)
    assert want.roots != list(store.roots) and want.roots[0] == store.roots[1]


@pytest.mark.parametrize("ids", [[100 + 3 * d + k for d in range(0, 75, 2) for k in (0, 2)] + [103, 104, 105],
                                 [100 + 3 * d + k for d in range(75) for k in (0, 1)], ids_of(CHAIN)], ids=["chain", "collapses", "all"])
def test_the_chain_of_75_levels(hand, ids):
    delete_and_compact(hand, make_store(hand, [CHAIN, TREE]), ids, 4)


@pytest.fixture(scope="module")
def small64():
    """the dataset the helpers of the insert tests hang their hand-made views on (64 dimensions, Euclidean)"""
    ctx = Ctx(D.Euclidean, INS.DIMS, 2100)
    ctx.ds.route_ids, ctx.ds.queries, ctx.ds.cand = ctx.ids[::7], ctx.queries, ctx.cand
    yield ctx
    ctx.close()


def test_delete_compact_insert_graft_compact(small64):
    ctx, ds = small64, small64.ds
    base = INS.make_store(INS.BASE, spread=10)
    ix, dense = ctx.index_of(base)
    try:
        deleted = [1, 2, 3, 4, 5, 6, 34, 35]
        after = clone(base)
        after.apply_delta(ix.delete_items(np.array(deleted, dtype=np.uint32), 2), dense)
        same_store(after, host_delete(base, deleted, 2))
        assert len(after.nodes) < len(base.nodes) and after.nodes[80][0] == "D"
        compact_and_check(ctx, ix, after)
        dense = INS.index_of_map(after)
        # insert: neither slots nor rows change, the index stays the fresh one
        ids = np.arange(1000, 1012, dtype=np.uint32)
        mid, _ = INS.host_insert(ds, after, ids, SEEDS)
        got = clone(after)
        got.apply_delta(ix.insert_items(ids, SEEDS[:len(after.roots)]), dense)
        same_store(got, mid)
        exact(ctx, ix, mid)
        # graft: the rows are full (normals_cap == n_normals), so the new plane makes them grow
        fp = ix.footprint()
        assert fp["normals_cap"] == fp["n_normals"] >= 1
        want, ix, dense, new_dense, view, keep, targets, new_index = INS.graft_case(ds, mid, [(80, INS.SUB3, [40, 41])], ix_dense=(ix, dense))
        ix.graft(view, targets, new_index)
        INS.same_index(ds, ix, new_dense, want, SEEDS, strict=True)
        fp2 = ix.footprint()
        assert fp2["n_normals"] == fp["n_normals"] + 1 and fp2["normals_cap"] >= 2 * fp["normals_cap"] and fp2["free_slots"] == 0
        before, m, stats = compact_and_check(ctx, ix, want)  # the new row is behind the others, its node is not
        assert stats["normals_cap_after"] == fp2["n_normals"] and stats["nodes_after"] == stats["nodes_before"]
    finally:
        ix.close()


def test_the_count_on_the_device_finds_nothing_to_do(small64):
    """a graft into spare rows, on an index without holes, of a plane whose node follows every other: the host cannot know that
    the index is still the fresh one, the counting pass finds it, and its scratch goes back"""
    ctx, ds = small64, small64.ds
    base = INS.make_store([[1, 2, 3, 4, 5, 6]])
    want, ix, dense, new_dense, view, keep, targets, new_index = INS.graft_case(ds, base, [(0, INS.SUB3, [1, 2])])
    try:
        assert ix.footprint()["normals_cap"] == 1 and ix.footprint()["n_normals"] == 0
        ix.graft(view, targets, new_index)
        live0 = _lib.device_cache_stats(0)[0]
        stats, m = ix.compact(want_map=True)
        assert stats["moved"] == 0 and m.tolist() == [0, 1, 2] and _lib.device_cache_stats(0)[0] == live0
        assert stats["normals_after"] == stats["normals_cap_after"] == 1 and stats["nodes_after"] == 3
        exact(ctx, ix, want)
    finally:
        ix.close()


# ---- 2. row widths -----------------------------------------------------------------------------------------------------

class Forest:
    """n rows of `dims` dimensions, a built forest of `n_trees` trees at split_after 8 as a TreeStore"""

    def __init__(self, dist, dims, n, n_trees, seed=21):
        self.ctx = Ctx(dist, dims, n, seed=seed, queries=16)
        self.seeds = list(range(11, 11 + n_trees))
        self.split_after = 8
        forest = self.ctx.ds.build_forest(self.seeds, split_after=self.split_after)
        self.store = TreeStore()
        self.store.roots = [self.store.next_id() for _ in self.seeds]
        for t, root in enumerate(self.store.roots):
            self.store.import_tree(forest, t, root_id=root)
        forest.close()
        self.perm = np.random.default_rng(seed).permutation(self.ctx.ids)
        self.want = {}

    def after(self, count):
        """the host's store after the first `count` ids of the permutation are deleted (computed once)"""
        if count not in self.want:
            self.want[count] = host_delete(self.store, self.perm[:count], self.split_after)
        return self.want[count]


WIDTHS = [("Cosine", 32), ("Cosine", 96), ("Cosine", 768), ("Cosine", 800), ("DotProduct", 32), ("DotProduct", 96), ("DotProduct", 768),
          ("DotProduct", 800), ("BinaryQuantizedEuclidean", 64), ("BinaryQuantizedEuclidean", 768)]


@pytest.mark.parametrize("dist_name,dims", WIDTHS, ids=[f"{w[0]}-{w[1]}" for w in WIDTHS])
def test_row_widths(dist_name, dims):
    f = Forest(getattr(D, dist_name), dims, 300, 2)
    try:
        info = f.ctx.index_of(f.store)
        info[0].close()
        want, before, m, stats = delete_and_compact(f.ctx, f.store, f.perm[:150], f.split_after, seeds=f.seeds)
        assert 0 < stats["normals_after"] < stats["normals_before"] and stats["nodes_after"] < stats["nodes_before"]
        rows = before["normal_rows"]
        assert rows.shape[1] == {32: 128, 96: 384, 768: 3072, 800: 3200}[dims] if dist_name != "BinaryQuantizedEuclidean" else \
            rows.shape[1] == {64: 16, 768: 96}[dims]
        assert before["normal_headers"].shape[1] == (2 if dist_name == "DotProduct" else 1)
    finally:
        f.ctx.close()


# ---- 3. past one scan tile and one launch ------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["Euclidean", "BinaryQuantizedEuclidean"])
def forest(request):
    f = Forest(getattr(D, request.param), 64, 20_000, 3)
    assert len(f.store.nodes) > 4096  # the scans over the node slots leave one tile
    yield f
    f.ctx.close()


@pytest.mark.parametrize("launch_max", [None, 1000], ids=["one-launch", "launches-of-1000"])
@pytest.mark.parametrize("share", [0.01, 0.10, 0.50, 1.0])
def test_random_forest(forest, share, launch_max):
    f = forest
    count = int(round(f.ctx.n * share))
    want = f.after(count)
    ix, dense = f.ctx.index_of(f.store)
    try:
        got = clone(f.store)
        got.apply_delta(ix.delete_items(np.sort(f.perm[:count]), f.split_after), dense)
        same_store(got, want)
        fp = ix.footprint()
        assert fp["free_slots"] == len(f.store.nodes) - len(want.nodes) > 0 and fp["n_normals"] > fp["live_normals"]
        if launch_max is not None:
            assert fp["n_nodes"] > 3 * launch_max
            assert share == 1.0 or fp["live_normals"] > 3 * launch_max
        with _lib.tuning(**({} if launch_max is None else {"AH_LAUNCH_MAX_ITEMS": launch_max})):
            before, m, stats = compact_and_check(f.ctx, ix, want, seeds=f.seeds)
        if share == 1.0:  # every root is an empty Descendants node and no row is live
            assert len(want.nodes) == 3 and all(nd[0] == "D" and nd[1].size == 0 for nd in want.nodes.values())
            assert stats["normals_after"] == 0 and stats["normals_cap_after"] == 1 and stats["nodes_after"] == 3
    finally:
        ix.close()


# ---- 4. chained builds -------------------------------------------------------------------------------------------------------

def test_three_chained_builds_with_and_without_compaction():
    w = INS.World(D.Euclidean, 8)
    ctx = Ctx(w.dist, INS.DIMS, INS.N, world=w)
    hosts, store = [], w.store
    for k in range(3):
        ids = w.updated(0.10, first=k * (INS.N // 20))
        hosts.append((store, ids, INS.host_cycle(w, store, ids, 100 * (k + 1))))
        store = hosts[-1][2][1]
    ix, dense = ctx.index_of(w.store)
    plain, pdense = ctx.index_of(w.store)
    try:
        dead = []
        for start, ids, host in hosts:
            assert host[2], "no node outgrew split_after: the graft was not exercised"
            dense = INS.device_cycle(w, ix, dense, start, ids, host)
            pdense = INS.device_cycle(w, plain, pdense, start, ids, host)
            fp = ix.footprint()
            assert fp["n_normals"] > fp["live_normals"]
            compact_and_check(ctx, ix, host[1], seeds=w.seeds)
            assert dense == INS.index_of_map(host[1])  # (a graft has renumbered already: the compaction moved rows only)
            fp = ix.footprint()
            assert fp["n_normals"] - fp["live_normals"] == 0
            pf = plain.footprint()
            dead.append(pf["n_normals"] - pf["live_normals"])
            assert pf["live_normals"] == fp["live_normals"] and pf["device_bytes"] > fp["device_bytes"]
        assert 0 < dead[0] < dead[1] < dead[2], dead
        INS.same_index(w.ds, plain, pdense, hosts[-1][2][1], w.seeds, w.dist, strict=True)  # (correct, only larger)
    finally:
        ix.close()
        plain.close()
        for _s, _i, h in hosts:
            if h[3] is not None:
                h[3].close()
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        w.ds.close()


# ---- 5. refusals leave the index unchanged --------------------------------------------------------------------------------------

def test_refusals_leave_the_index_unchanged(hand):
    L = _lib.lib()
    assert L.ah_index_compact(None, None, None) == INVALID and b"index is NULL" in L.ah_last_error()
    assert L.ah_index_footprint_get(None, C.byref(_lib.AhIndexFootprint())) == INVALID and b"index is NULL" in L.ah_last_error()
    store = make_store(hand, [T(40), T(60), TREE])
    ix, dense = hand.index_of(store)
    try:
        ix.delete_items(np.array(sorted(ids_of(T(40)) + [17, 18]), dtype=np.uint32), 4)
        want = host_delete(store, ids_of(T(40)) + [17, 18], 4)
        assert L.ah_index_footprint_get(ix._h, None) == INVALID and b"out is NULL" in L.ah_last_error()
        before, fp = ix.export(), ix.footprint()
        assert fp["free_slots"] > 0 and fp["n_normals"] > fp["live_normals"]
        f = ix.make_filter(hand.cand, sorted=True)
        refused(lambda: ix.compact(), "live filters")
        assert ix.footprint() == fp  # (legal under a live filter)
        same_arrays(before, ix.export())
        f.close()
        ix.suspend()
        refused(lambda: ix.compact(), "suspended")
        refused(lambda: ix.footprint(), "suspended")
        ix.resume()
        same_arrays(before, ix.export())
        assert ix.footprint() == fp
        compact_and_check(hand, ix, want)
    finally:
        ix.close()


# ---- 6. allocation failures ---------------------------------------------------------------------------------------------------

def test_compact_and_footprint_survive_every_allocation_failure(forest):
    f = forest
    count = f.ctx.n // 10
    want = f.after(count)
    ix, dense = f.ctx.index_of(f.store)
    try:
        ix.delete_items(np.sort(f.perm[:count]), f.split_after)
        q = f.ctx.queries[:8]

        def probe():
            e = ix.export()
            return ix.search(10, queries=q, search_k=500, raw=True) + (
                ix.route_items(f.ctx.ids[::40], f.seeds), e["nodes"].view(np.uint8), e["roots"], e["descendants"], e["normal_rows"],
                e["normal_headers"])
        fp = INS.sweep(lambda: ix.footprint(), probe, 1, need_oom=False)
        assert fp["free_slots"] == len(f.store.nodes) - len(want.nodes)
        # the scratch of the count, nodes, roots, rows, headers, the old row of every new row (+ the host's vector)
        stats, m = INS.sweep(lambda: ix.compact(want_map=True), probe, 6)
        assert stats["moved"] == 1 and stats["nodes_after"] == len(want.nodes)
        exact(f.ctx, ix, want, seeds=f.seeds)
        assert ix.compact()["moved"] == 0
    finally:
        ix.close()


# ---- 7. Writer ----------------------------------------------------------------------------------------------------------------

def run_writer(dist, device_compact_on, hook=None, dims=24):
    n0, builds = 900, 5
    g = np.random.default_rng(5)
    vecs = g.standard_normal((n0 * (builds + 1), dims)).astype(np.float32)
    db = I.Database(dist)
    w = I.Writer(db, 0, dims)
    st = w._st
    snaps = []
    for i in range(n0):
        w.add_item(i, vecs[i])
    for k in range(builds + 1):
        if k:  # half of the items get a new vector
            for i in g.choice(n0, n0 // 2, replace=False):
                w.add_item(int(i), vecs[k * n0 + int(i)])
        b = w.builder(random.Random(40 + k)).n_trees(5)
        b.device_compact = device_compact_on
        before = st.device_compactions
        if hook is not None:
            hook(k, st)
        b.build()
        reader = I.Reader.open(db, 0)
        qs = vecs[[1, 500, 950, 1300]]
        fresh_fp = None
        if st.device_compactions > before:  # a build that compacted: the resident index is the fresh one
            view, keep = st.trees.to_view(dist, dims)
            fresh = Index(st.dataset, None, view=view)
            assert st.index.footprint() == fresh.footprint() and st._keep[4] == keep[4]
            same_arrays(st.index.export(), fresh.export())
            fresh.close()
            fresh_fp = True
        snaps.append((clone(st.trees), copy.deepcopy(st.metadata), [reader.nns(10).search_k(300).by_vector(q) for q in qs],
                      reader.nns(5).by_item(st.metadata["items"][3]), reader.stats(), st.device_compactions, st.device_inserts,
                      st.index_uploads, fresh_fp, st.index.footprint()))
    st.index.close()
    st.dataset.close()
    return snaps


@pytest.mark.parametrize("dist_name,dims", [("Euclidean", 24), ("BinaryQuantizedEuclidean", 64)])
def test_writer_compacts_and_builds_the_same_trees(dist_name, dims):
    dist = getattr(D, dist_name)
    on, off = run_writer(dist, True, dims=dims), run_writer(dist, False, dims=dims)
    assert on[0][9]["n_normals"] > 100  # (the forest has planes to orphan)
    assert [s[5] for s in off] == [0] * len(off) and on[-1][5] > 0
    assert [s[6] for s in on] == [s[6] for s in off] == list(range(len(on))) and [s[7] for s in on] == [s[7] for s in off] == [1] * len(on)
    for k, (a, b) in enumerate(zip(on, off)):
        same_store(a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3] and a[4] == b[4], k
    # without the compaction the waste passes the threshold and stays; with it no build ends above it
    assert any(I.compaction_due(s[9]) for s in off)
    for s in on:
        assert not I.compaction_due(s[9])


def test_writer_build_with_a_filter_alive_skips_the_compaction(monkeypatch):
    """A refusal of the compaction is not a failure of the build: a filter made on the resident index between the build's last
    step and the compaction makes ah_index_compact refuse; the build ends as without it."""
    filters, real = [], Index.footprint

    def footprint(self):
        if not filters:
            filters.append(self.make_filter(range(0, 900, 2)))
        return real(self)
    monkeypatch.setattr(I, "compaction_due", lambda fp: True)

    def hook(k, st):
        if k == 2:
            monkeypatch.setattr(Index, "footprint", footprint)
        elif k == 3:
            monkeypatch.setattr(Index, "footprint", real)
    on, off = run_writer(D.Euclidean, True, hook), run_writer(D.Euclidean, False)
    assert len(filters) == 1
    assert [s[5] for s in on] == [0, 1, 1, 2, 3, 4]  # build 2 was refused its compaction, and only that
    for k, (a, b) in enumerate(zip(on, off)):
        same_store(a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3] and a[4] == b[4], k
