"""Filters across index maintenance: ah_filter_suspend, ah_filter_resume_batch, ah_index_filters_suspended.

The yardstick everywhere is the existing path: ah_filter_create on the index AS IT IS NOW from the ascending list of
S = ((old set - remove) | add) & [0, largest stored id], compared through Filter.export() (length, bitmap words, per-node
counts) and info() (`stored`; `listed` is the number of set bits).  The numpy model of tests/test_filter_resume_cpu.py predicts
the words and ah_filter_resume_stats.  The worlds are a few thousand items, 3 trees, 8 dimensions, split_after 16."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import arroy_amd.index as I
from arroy_amd import Dataset, Index, _lib, shard
from arroy_amd import distances as D
from audit_model import Case
from test_filter_resume_cpu import GROUP, groups_of, padded_words, resume_model, words_of
from test_gpu_search_filters import OOM, sweep, sweep_once

pytestmark = pytest.mark.gpu

DIMS, TREES, SPLIT_AFTER = 8, 3, 16
SEEDS = shard.tree_seeds(23, range(TREES + 2))


def u32(a):
    return np.ascontiguousarray(sorted(set(int(x) for x in a)), dtype=np.uint32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def popcount(words):
    return int(np.bitwise_count(words).sum(dtype=np.uint64))


def vectors(ids):
    """A vector per id that depends on the id alone: an id keeps its row through every update."""
    ids = np.asarray(ids, dtype=np.int64)
    return (np.sin(ids[:, None] * np.arange(1, DIMS + 1)[None, :] * 0.37) + ((ids[:, None] * 7 + np.arange(DIMS)[None, :]) % 11) * 0.1).astype(np.float32)


def expected(old, remove, add, max_id):
    return u32(i for i in (set(old) - set(remove)) | set(add) if i <= max_id)


class World:
    def __init__(self, ids):
        self.ids = set(int(i) for i in ids)
        arr = u32(self.ids)
        self.ds = Dataset(D.Euclidean, DIMS, arr.size)
        self.ds.upload_vectors(arr, vectors(arr))
        self.ds.finalize()
        self.forest = self.ds.build_forest(SEEDS[:TREES], split_after=SPLIT_AFTER)
        self.index = self.ds.create_index(self.forest)

    @property
    def max_id(self):
        return max(self.ids)

    def update(self, remove, add):
        """The whole cycle of an incremental build around the suspended filters: the index gives up the dataset, the dataset is
        updated, the index takes it again, the removed ids leave its trees and the new ones are routed into them."""
        remove, add = u32(remove), u32(add)
        self.index.suspend(keep_filters=True)
        self.ds.update_vectors(remove, add, vectors(add))
        self.index.resume()
        self.ids = (self.ids - set(remove.tolist())) | set(add.tolist())
        if remove.size:
            self.index.delete_items(remove, SPLIT_AFTER)
        if add.size:
            self.index.insert_items(add, SEEDS[:self.index.export_info()["n_trees"]])

    def same_as_list(self, got, want_ids, what):
        """`got` is bit for bit the filter ah_filter_create makes now of want_ids; returns its export."""
        with self.index.make_filter(want_ids, sorted=True) as want:
            ge, we = got.export(), want.export()
            gi, wi = got.info(), want.info()
        assert ge["len_bits"] == we["len_bits"] == self.max_id + 1, (what, ge["len_bits"], we["len_bits"])
        assert np.array_equal(ge["bits"], we["bits"]), what
        assert ge["leaf_kept"].size == self.index.export_info()["n_nodes"] and np.array_equal(ge["leaf_kept"], we["leaf_kept"]), what
        assert gi["stored"] == wi["stored"] == len(self.ids & set(want_ids.tolist())), (what, gi, wi)
        assert gi["listed"] == popcount(ge["bits"]) == want_ids.size, (what, gi)
        return ge

    def close(self):
        self.index.close()  # (closes its filters, the suspended ones too)
        self.forest.close()
        self.ds.close()


def suspend_all(fs):
    for f in fs:
        f.suspend()
        assert f.suspended


# ---- length edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first,then", [(2046, 2048), (2048, 2046)], ids=["2046_to_2048", "2048_to_2046"])
def test_the_largest_id_crosses_a_word_and_the_padding_unit(first, then):
    """len_bits 2047 <-> 2049: across a 32-bit word and across the 64-word (2048-bit) padding unit.  Old bits at and above the new
    length vanish, added ids above it are skipped, and NOT / OR of the resumed filter (ah_filter_combine reads the operands' words
    whole, padding included) equal the list-made ones: no dirty tail."""
    w = World(range(first + 1))
    try:
        olds = [u32(range(0, first + 1, 3)), u32(range(first + 1)), u32([first - 1, first]), u32([])]
        fs = [w.index.make_filter(o, sorted=True) for o in olds]
        other = u32(range(1, min(first, then) + 1, 7))
        before = [f.info() for f in fs]
        suspend_all(fs)
        assert [f.info() for f in fs] == before  # the old listed / stored, and the block it still holds
        if then > first:
            w.update([], range(first + 1, then + 1))
        else:
            w.update(range(then + 1, first + 1), [])
        assert w.max_id == then
        edits = [([5, 2045], [2044, 2047, 2048, 2049, 5000]), None, ([], [2046]), ([7], [2045, 2048])]
        st = w.index.resume_filters(fs, edits, want_stats=True)
        assert (st["filters"], st["groups"], st["words"]) == (4, 1, 4 * padded_words(then + 1)), st
        removed = added = 0
        for f, old, e in zip(fs, olds, edits):
            rm, add = e if e is not None else ([], [])
            want = expected(old, rm, add, then)
            ge = w.same_as_list(f, want, (first, then, old.size))
            model, listed, r, a = resume_model(words_of(old, first + 1), first + 1, then + 1, rm, add)
            assert np.array_equal(ge["bits"], model[:ge["bits"].size]) and listed == want.size
            removed, added = removed + r, added + a
            inv, both = ~f, f | w.index.make_filter(other, sorted=True)
            w.same_as_list(inv, np.setdiff1d(np.arange(then + 1, dtype=np.uint32), want).astype(np.uint32), "not")
            w.same_as_list(both, np.union1d(want, other).astype(np.uint32), "or")
        assert (st["ids_removed"], st["ids_added"]) == (removed, added), st
    finally:
        w.close()


# ---- both id kinds, the group hand-over, the tunable --------------------------------------------------------------------------

def group_case(w, n, pool, unstored):
    """n filters over the stored ids `pool`: an empty one, a full one, two equal ones, random ones; distinct edits each, filter 1
    (the full one) without."""
    rng = np.random.default_rng(n)
    olds, edits = [], []
    for i in range(n):
        if i == 0:
            old = pool[:0]
        elif i == 1:
            old = pool
        elif i in (2, 3):
            old = pool[::3]
        else:
            old = pool[rng.random(pool.size) < rng.uniform(0.01, 0.6)]
        olds.append(u32(old))
        rm = rng.choice(pool, 5 + i % 7, replace=False).tolist() + unstored[i % 3:i % 3 + 2]
        add = rng.choice(pool, 3 + i % 5, replace=False).tolist() + unstored[i % 4:i % 4 + 1] + [rm[0]]  # (rm[0]: in both lists)
        edits.append(None if i == 1 else (rm, add) if i % 5 else (None, add))
    return olds, edits


@pytest.mark.parametrize("kind", ["identity", "sparse"])
def test_groups_of_filters_resume_on_identity_and_sparse_ids(kind):
    """n = 1, G, G + 1 and 2G + 1 filters in one call, after a delete on the index; identity ids (`stored` is the popcount) and
    sparse ids with listed ids that are not stored (`stored` through the dataset's id array).  AH_FILTER_RESUME_GROUP = 1 and 5
    (a pass per filter; groups filled up to 16 with copies of their first filter) give the same filters in more passes, and so
    does a budget too small for a group's bitmaps side by side (AH_FILTER_RESUME_MIXED_MB = 0: a pass per filter)."""
    n_items = 2500
    ids = np.arange(n_items, dtype=np.uint32) if kind == "identity" else (np.arange(n_items, dtype=np.uint64) * 7 + np.arange(n_items) % 3).astype(np.uint32)
    w = World(ids)
    try:
        unstored = [int(ids[-1]) + 1, int(ids[-1]) + 50, 2**31 + 5, 0xFFFFFFFF] if kind == "identity" else \
            [int(ids[10]) + 3, int(ids[500]) + 3, int(ids[-1]) + 9, 0xFFFFFFFF, int(ids[-2]) + 3]
        for n, group, mixed_mb in ((1, GROUP, 256), (GROUP, GROUP, 256), (GROUP + 1, GROUP, 256), (2 * GROUP + 1, GROUP, 256),
                                   (GROUP + 1, 1, 256), (7, 5, 256), (GROUP + 1, GROUP, 0)):
            olds, edits = group_case(w, n, ids, unstored)
            fs = [w.index.make_filter(o, sorted=True) for o in olds]
            st0 = w.index.filter_stats()
            suspend_all(fs)
            assert w.index.filters_suspended() == n and w.index.filter_stats()["filters_alive"] == st0["filters_alive"] - n
            gone = ids[n::97]
            w.index.delete_items(gone, SPLIT_AFTER)  # (maintenance under suspended filters; the ids stay rows of the dataset)
            ex = w.index.export(normals=False)
            leaf = (ex["nodes"]["kind"] == 1) & (ex["nodes"]["count"] > 0)
            with _lib.tuning(AH_FILTER_RESUME_GROUP=group, AH_FILTER_RESUME_MIXED_MB=mixed_mb):
                st = w.index.resume_filters(fs, edits, want_stats=True)
            n_groups = groups_of(n, group if mixed_mb else 1)
            assert (st["filters"], st["groups"]) == (n, n_groups) and st["words"] == n * padded_words(w.max_id + 1), st
            assert st["leaves"] == int(leaf.sum()) and st["ids_walked"] == n_groups * int(ex["nodes"]["count"][leaf].sum()), st
            st1 = w.index.filter_stats()
            assert w.index.filters_suspended() == 0 and st1["filters_alive"] == st0["filters_alive"]
            assert st1["filters_created"] == st0["filters_created"] and st1["leaf_kept_passes"] == st0["leaf_kept_passes"] + n_groups
            removed = added = 0
            for i, (f, old, e) in enumerate(zip(fs, olds, edits)):
                rm, add = (e[0] or [], e[1] or []) if e is not None else ([], [])
                w.same_as_list(f, expected(old, rm, add, w.max_id), (kind, n, group, i))
                _, _, r, a = resume_model(words_of(old, w.max_id + 1), w.max_id + 1, w.max_id + 1, rm, add)
                removed, added = removed + r, added + a
                assert not f.suspended
            assert (st["ids_removed"], st["ids_added"]) == (removed, added), st
            for f in fs:
                f.close()
            w.index.insert_items(gone, SEEDS[:TREES])  # the world as it was
    finally:
        w.close()


# ---- leaf sizes -----------------------------------------------------------------------------------------------------------------

def test_every_leaf_size_between_split_nodes_and_free_slots():
    """Leaves of 0, 1, 7, 8, 9, 63, 64, 65 and 300 ids (one octet step is 32 ids: none, one partial, exactly two, two and a part,
    ten) in a hand-made forest of two trees, split nodes in between; then again after a delete has emptied two leaves, which
    leaves free slots in the node array."""
    sizes = [0, 1, 7, 8, 9, 63, 64, 65, 300]
    total = sum(sizes)
    rng = np.random.default_rng(2)
    trees, ranges = [], []
    for t in range(2):
        order = rng.permutation(total)
        leaves, at = [], 0
        for c in (sizes if t == 0 else sizes[::-1]):
            leaves.append(sorted(order[at:at + c].tolist()))
            at += c
        ranges.append(leaves)
        trees.append(functools.reduce(lambda acc, leaf: (acc, leaf, None), leaves[1:], leaves[0]))
    case = Case(trees)
    ids = np.arange(total, dtype=np.uint32)
    ds = Dataset(D.Euclidean, DIMS, total)
    ds.upload_vectors(ids, vectors(ids))
    ds.finalize()
    view, keep = case.view(D.Euclidean, DIMS)
    index = Index(ds, None, view=view)
    try:
        ex = index.export(normals=False)
        assert sorted(ex["nodes"]["count"][ex["nodes"]["kind"] == 1].tolist()) == sorted(sizes * 2) and (ex["nodes"]["kind"] == 2).sum() == 16
        olds = [u32(ids[::2]), u32(ids), u32([]), u32(ranges[0][8]), u32(ranges[1][3] + ranges[0][5][:40])]
        fs = [index.make_filter(o, sorted=True) for o in olds]
        for step in range(2):
            suspend_all(fs)
            if step == 1:
                index.delete_items(u32(ranges[0][2] + ranges[0][6]), 1)
                ex = index.export(normals=False)
                assert (ex["nodes"]["kind"] == 0).sum() >= 2  # free slots, split nodes and leaves side by side
            edits = [([1, 2, 3], [4, 5, 6, total + 7]), None, (None, ranges[0][7]), (ranges[0][8][:150], None), ([], [])]
            index.resume_filters(fs, edits)
            for k, (f, old, e) in enumerate(zip(fs, olds, edits)):
                rm, add = (e[0] or [], e[1] or []) if e is not None else ([], [])
                olds[k] = expected(old, rm, add, total - 1)
                with index.make_filter(olds[k], sorted=True) as want:
                    ge, we = f.export(), want.export()
                    assert np.array_equal(ge["bits"], we["bits"]) and np.array_equal(ge["leaf_kept"], we["leaf_kept"]), (step, k)
                    assert f.info()["stored"] == want.info()["stored"] == olds[k].size
                leaf = ex["nodes"]["kind"] == 1
                assert ge["leaf_kept"][~leaf].sum() == 0 and ge["leaf_kept"].size == ex["nodes"].size
    finally:
        index.close()
        ds.close()
    del keep


# ---- after each maintenance call -------------------------------------------------------------------------------------------

def test_filters_resume_after_every_maintenance_call_and_dataset_update():
    w = World(range(3000))
    forests = []
    try:
        rng = np.random.default_rng(9)
        olds = [u32(range(0, 3000, 2)), u32(rng.choice(3000, 150, replace=False)), u32(range(3000)), u32(range(2900, 3000))]
        fs = [w.index.make_filter(o, sorted=True) for o in olds]

        def cycle(what, op, edits=None):
            suspend_all(fs)
            op()
            st = w.index.resume_filters(fs, edits, want_stats=True)
            for k, (f, old) in enumerate(zip(fs, olds)):
                rm, add = edits[k] if edits is not None and edits[k] is not None else ([], [])
                olds[k] = expected(old, rm or [], add or [], w.max_id)
                w.same_as_list(f, olds[k], (what, k))
            return st

        gone = u32(range(5, 3000, 3))
        n0 = w.index.export_info()["n_nodes"]
        cycle("delete", lambda: w.index.delete_items(gone, SPLIT_AFTER))
        assert w.index.footprint()["free_slots"] > 0

        def compact():
            stats, new_of_old = w.index.compact(want_map=True)
            assert stats["moved"] and not np.array_equal(new_of_old, np.arange(new_of_old.size))  # the slots are renumbered
        cycle("compact", compact)
        assert w.index.export_info()["n_nodes"] < n0 and w.index.footprint()["free_slots"] == 0

        def insert_and_graft():
            w.index.insert_items(gone, SEEDS[:TREES])
            forests.append(w.ds.build_forest(SEEDS[TREES:TREES + 1], split_after=SPLIT_AFTER))
            w.index.graft(forests[-1].view_struct(), [_lib.NEW_ROOT])
        cycle("insert + graft", insert_and_graft, [([1, 2], [5, 8]), None, None, ([2999], [3, 4000])])
        assert w.index.export_info()["n_trees"] == TREES + 1
        cycle("drop", lambda: w.index.drop_trees(2))
        assert w.index.export_info()["n_trees"] == TREES - 1
        # the whole cycle of an incremental build: a grown dataset (ids 3000 .. 3099 and the host's adds), then a shrunk one
        new = list(range(3000, 3100))
        st = cycle("grown", lambda: w.update([10, 11, 500], new), [([10, 11], new[::2]), ([500], [3099, 3100]), ([10, 11, 500], new), None])
        assert st["words"] == 4 * padded_words(3100) and w.max_id == 3099
        cycle("shrunk", lambda: w.update(range(2048, 3100), []), [(range(2048, 3100), None)] * 4)
        assert w.max_id == 2047 and fs[3].info()["listed"] == 1 and fs[2].info()["stored"] == len(w.ids)  # (fs[3]: id 3 is left)
    finally:
        w.close()
        for f in forests:
            f.close()


# ---- search parity ------------------------------------------------------------------------------------------------------------

def test_searches_under_a_resumed_filter_equal_those_under_a_fresh_one_and_under_the_list():
    w = World(range(3000))
    try:
        rng = np.random.default_rng(4)
        nq = 24
        queries = (vectors(rng.choice(3000, nq, replace=False)) + rng.standard_normal((nq, DIMS)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
        olds = [u32(range(0, 3000, 2)), u32(rng.choice(3000, 90, replace=False)), u32(range(1000, 2600))]  # shares 0.5, 0.03, 0.53
        fs = [w.index.make_filter(o, sorted=True) for o in olds]
        suspend_all(fs)
        w.update(range(2800, 3000), range(3000, 3050))
        edits = [(range(2800, 3000, 2), range(3000, 3050, 2)), ([int(x) for x in olds[1] if x >= 2800], [3001, 3002]), ([1000, 1001], [7, 3049])]
        w.index.resume_filters(fs, edits)
        lists = [expected(o, rm, add, w.max_id) for o, (rm, add) in zip(olds, edits)]
        fresh = [w.index.make_filter(x, sorted=True) for x in lists]
        for f, g, lst in zip(fs, fresh, lists):
            res = []
            for cand in (f, g, lst):
                w.index.stats(reset=True)
                kw = dict(candidates_sorted=True) if cand is lst else {}
                out = [w.index.search(10, queries=queries[i:i + 1], search_k=200, raw=True, candidates=cand, **kw) for i in range(4)]
                out.append(w.index.search(10, queries=queries, search_k=200, raw=True, candidates=cand, **kw))
                res.append((out, w.index.stats()))
            for other in res[1:]:
                for x, y in zip(res[0][0], other[0]):
                    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(x, y))
            assert res[0][1] == res[1][1]  # resumed and fresh: every counter of ah_search_stats
            path = lambda s: {k: v for k, v in s.items() if k != "leaf_kept_passes"}  # noqa: E731 (the list way makes its counts per call)
            assert path(res[0][1]) == path(res[2][1]), (res[0][1], res[2][1])
            assert res[0][1]["filtered_queries"] == nq + 4 and int(res[0][0][-1][2].sum()) > 0
        # one mixed call: every query under the resumed, under the fresh filter of the same set, and one unfiltered
        both = [x for pair in zip(fs, fresh) for x in pair]
        q2 = np.repeat(queries, 2, axis=0)
        slots = np.array([2 * (i % 3) + j for i in range(nq) for j in range(2)], dtype=np.uint32)
        for gmin in (1, 16, 1000):
            with _lib.tuning(AH_SEARCH_FILTER_GROUP_MIN=gmin):
                oi, od, oc = w.index.search(10, queries=q2, search_k=200, raw=True, filters=both, filter_of_query=slots)
            assert np.array_equal(oi[0::2], oi[1::2]) and np.array_equal(bits(od[0::2]), bits(od[1::2])) and np.array_equal(oc[0::2], oc[1::2]), gmin
            for i in range(nq):
                one = w.index.search(10, queries=queries[i:i + 1], search_k=200, raw=True, candidates=lists[i % 3], candidates_sorted=True)
                assert np.array_equal(oi[2 * i], one[0][0]) and np.array_equal(bits(od[2 * i]), bits(one[1][0])) and oc[2 * i] == one[2][0], (gmin, i)
    finally:
        w.close()


# ---- lifecycle ------------------------------------------------------------------------------------------------------------------

def refused(fn, *words):
    with pytest.raises(_lib.ArroyHipError) as e:
        fn()
    assert e.value.status == 5, e.value
    for word in words:
        assert word in str(e.value), e.value


def test_maintenance_goes_through_under_a_suspended_filter_and_is_refused_under_a_live_one():
    """What the feature is for: with a filter present, delete_items / compact / ah_index_suspend could only be had by destroying
    it.  Suspended, it lets them through and resumes correct; alive, it still refuses them with "live filters"."""
    w = World(range(2000))
    try:
        old = u32(range(0, 2000, 3))
        f = w.index.make_filter(old, sorted=True)
        gone = u32(range(1, 2000, 4))
        refused(lambda: w.index.delete_items(gone, SPLIT_AFTER), "live filters")
        refused(lambda: w.index.compact(), "live filters")
        assert _lib.lib().ah_index_suspend(w.index._h) == 5 and b"live filters" in _lib.lib().ah_last_error()
        f.suspend()
        w.index.delete_items(gone, SPLIT_AFTER)
        assert w.index.compact()["moved"]
        _lib.check(_lib.lib().ah_index_suspend(w.index._h))
        w.index.resume()
        w.index.resume_filters([f])
        w.same_as_list(f, old, "after delete, compact, suspend")
        refused(lambda: w.index.delete_items(u32([0, 3]), SPLIT_AFTER), "live filters")
    finally:
        w.close()


def test_lifecycle_refusals_and_counters():
    w = World(range(2000))
    L = _lib.lib()
    other = None
    try:
        dev = w.ds.device
        other = Index(w.ds, w.forest)
        w.index.make_filter([1, 2]).close()  # (a first call warms the calling thread's context up)
        live0, _ = _lib.device_cache_stats(dev)
        a, b = w.index.make_filter(range(0, 2000, 2)), w.index.make_filter(range(0, 2000, 5))
        info = a.info()
        a.suspend()
        assert a.info() == info and a.suspended and not b.suspended
        assert w.index.filters_suspended() == 1 and w.index.filter_stats()["filters_alive"] == 1
        # refused by name wherever a filter is read
        refused(lambda: w.index.search(5, queries=vectors([3]), search_k=50, candidates=a), "filters[0] is suspended")
        refused(lambda: w.index.search(5, queries=vectors([3, 4]), search_k=50, filters=[b, a], filter_of_query=[0, 1]), "filters[1] is suspended")
        refused(lambda: b & a, "operands[1] is suspended")
        refused(lambda: ~a, "operands[0] is suspended")
        refused(a.export, "suspended")
        refused(a.suspend, "suspended")
        # resume: a live filter, a duplicate, a filter of another index, a suspended index — each by its position
        refused(lambda: w.index.resume_filters([a, b]), "filters[1] is not suspended")
        refused(lambda: w.index.resume_filters([a, a]), "filters[1] names the same filter as filters[0]")
        c = other.make_filter(range(10))
        c.suspend()
        arr = (C.c_void_p * 2)(a._handle(), c._handle())
        assert L.ah_filter_resume_batch(arr, None, 2, None) == 5 and b"filters[1] belongs to another index" in L.ah_last_error()
        b.close()
        w.index.suspend(keep_filters=True)  # (a is suspended already: left alone)
        refused(lambda: w.index.resume_filters([a]), "the index is suspended")
        refused(lambda: w.index.make_filter([1]), "suspended")
        w.index.resume()
        assert a.suspended and a.info() == info and w.index.filters_suspended() == 1  # every refusal left it as it was
        # the index cannot go while a suspended filter points at it; the filter can
        assert L.ah_index_destroy(w.index._h) == 5 and b"suspended filters" in L.ah_last_error() and b"live filter" not in L.ah_last_error()
        a.close()
        c.close()
        assert w.index.filters_suspended() == 0 == other.filters_suspended() and w.index.filter_stats()["filters_alive"] == 0
        # Index.suspend: the default closes the live filters, keep_filters suspends them; Index.close closes suspended ones too
        d, e = other.make_filter(range(50)), other.make_filter(range(70))
        d.suspend()
        other.suspend()
        assert d.suspended and not e._h
        other.resume()
        other.resume_filters([d])
        g = other.make_filter(range(30))
        other.suspend(keep_filters=True)
        assert d.suspended and g.suspended and other.filters_suspended() == 2
        other.resume()
        other.resume_filters([d])
        other.make_filter(range(3)).close()
        d.close()
        assert other.filters_suspended() == 1 and _lib.device_cache_stats(dev)[0] == live0 + g.info()["device_bytes"]
        other.close()
        other = None
        assert not g._h
    finally:
        if other is not None:
            other.close()
        w.close()


# ---- every allocation failing once --------------------------------------------------------------------------------------------

def test_suspend_and_resume_survive_every_allocation_failure():
    """The sweep of tests/test_gpu_faults.py (the library's own injection: a status by design, no device fault).  After each
    failure every filter is still suspended with its old info() and no counter has moved; a clean resume is then correct."""
    w = World(range(2500))
    try:
        n = GROUP + 1
        ids = np.arange(2500, dtype=np.uint32)
        olds, edits = group_case(w, n, ids, [2500, 2600, 9000, 0xFFFFFFFF])
        fs = [w.index.make_filter(o, sorted=True) for o in olds]
        w.index.resume_filters([])  # n == 0: nothing happens

        def resume():  # the world is put back by cleanup: every call of the sweep starts from n suspended filters
            st0 = (w.index.filter_stats(), w.index.filters_suspended())
            infos = [f.info() for f in fs]  # (after the first call that went through, the edits have been applied already)
            try:
                return w.index.resume_filters(fs, edits, want_stats=True)
            except _lib.ArroyHipError:
                left = _lib.tuning_get("AH_FAIL_ALLOC_AFTER")[0]
                _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
                assert all(f.suspended for f in fs) and [f.info() for f in fs] == infos
                assert (w.index.filter_stats(), w.index.filters_suspended()) == st0
                _lib.tuning_set("AH_FAIL_ALLOC_AFTER", left)
                raise

        def suspend_one():
            fs[0].suspend()
            return True
        seen = sweep(suspend_one, cleanup=lambda _: w.index.resume_filters([fs[0]]))
        assert all(s == OOM for s in seen), seen  # (the call allocates nothing on the device: at most a host allocation)
        assert not fs[0].suspended and w.index.filters_suspended() == 0
        suspend_all(fs)
        # Nothing leaks: a resume takes n recycled blocks and gives n back, and the allocator hands out blocks a little larger
        # than asked for, so the live bytes alone swing between two generations of blocks; live + idle cannot (nothing goes
        # back to the driver below the cache's budget)
        seen = sweep_once(resume, cleanup=lambda _: suspend_all(fs))
        held = sum(_lib.device_cache_stats(w.ds.device))
        again = sweep_once(resume, cleanup=lambda _: suspend_all(fs))
        assert sum(_lib.device_cache_stats(w.ds.device)) == held and again == seen
        assert len(seen) >= n + 2 and OOM in seen, seen  # a block per filter, the call's upload, host vectors
        assert all(f.suspended for f in fs)
        st = resume()
        assert st["groups"] == 2
        for i, (f, old, e) in enumerate(zip(fs, olds, edits)):
            rm, add = (e[0] or [], e[1] or []) if e is not None else ([], [])
            w.same_as_list(f, expected(old, rm, add, w.max_id), i)
    finally:
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        w.close()


# ---- ArroyBuilder.keep_filters -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep_filters", [True, False])
def test_an_incremental_build_keeps_the_filters_of_its_readers_suspended(monkeypatch, keep_filters):
    """keep_filters: two Reader filters alive at an incremental build are suspended, not closed; the end-of-build compaction runs;
    resumed, they equal fresh ones.  Without the flag the build closes them, as before."""
    dims, n = 24, 900
    g = np.random.default_rng(5)
    vecs = g.standard_normal((2 * n, dims)).astype(np.float32)
    db = I.Database(D.Euclidean)
    wr = I.Writer(db, 0, dims)
    st = wr._st
    for i in range(n):
        wr.add_item(i, vecs[i])
    wr.builder(random.Random(40)).n_trees(5).build()
    reader = I.Reader.open(db, 0)
    lists = [u32(range(0, n, 2)), u32(range(100, 400))]
    fs = [reader.make_filter(x) for x in lists]
    index = st.index
    for i in g.choice(n, n // 2, replace=False):
        wr.add_item(int(i), vecs[n + int(i)])
    monkeypatch.setattr(I, "compaction_due", lambda fp: True)
    b = wr.builder(random.Random(41)).n_trees(5)
    b.keep_filters = keep_filters
    before = st.device_compactions
    b.build()
    try:
        assert st.index is index and st.device_compactions == before + 1  # the resident index was kept and compacted
        if not keep_filters:
            assert not fs[0]._h and not fs[1]._h and index.filters_suspended() == 0
            return
        assert all(f.suspended for f in fs) and index.filters_suspended() == 2 and index.filter_stats()["filters_alive"] == 0
        index.resume_filters(fs)  # (the build changed vectors, not the set of ids: no delta)
        for f, x in zip(fs, lists):
            with index.make_filter(x, sorted=True) as want:
                ge, we = f.export(), want.export()
                assert ge["len_bits"] == we["len_bits"] and np.array_equal(ge["bits"], we["bits"]) and np.array_equal(ge["leaf_kept"], we["leaf_kept"])
                assert f.info()["stored"] == want.info()["stored"] == x.size
        hits = I.Reader.open(db, 0).nns(5).search_k(200).candidates(fs[1]).by_vector(vecs[150])
        assert hits and all(100 <= int(i) < 400 for i, _ in hits)
    finally:
        st.index.close()
        st.dataset.close()
