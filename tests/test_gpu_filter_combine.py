"""Filter expressions on the device (ah_filter_combine) and filters from bitmaps (ah_filter_create_bitmap).

The yardstick is always the existing path: ah_filter_create of the ascending id list numpy computes for the expression
(np.intersect1d / union1d / setdiff1d, the complement within [0, largest id]); tests/test_gpu_search_filters.py holds such
filters against the oracle.  The new filter's export (bitmap words, per-node counts) and `stored` must be identical to the
list-made filter's, `listed` must be the popcount, and ah_filter_combine_stats must be what `derive`
(tests/test_filter_combine_cpu.py) predicts from the operands' exported counts.

One exception, stated where it is made: on the world whose last id is u32::MAX the complement of a small set is a list of
2^32 - |a| ids (16 GiB), which no test can hand to ah_filter_create; NOT is checked there against numpy's complement of the
operand's exported words, against c - k per leaf and n - stored, and through `(NOT a) AND b`, which has a list."""
import ctypes as C
import functools

import numpy as np
import pytest

from arroy_amd import Index, _lib, roaring, shard
from arroy_amd import Dataset
from arroy_amd import distances as D
from test_filter_combine_cpu import AND, ANDNOT, NOT, OR, WALK, derive
from test_gpu_search_filters import OOM, sweep

pytestmark = pytest.mark.gpu

DIMS, TREES, SPLIT_AFTER = 24, 3, 16
U32_MAX = 0xFFFFFFFF
OP_NAME = {AND: "and", OR: "or", ANDNOT: "andnot", NOT: "not"}
# (name, rows, largest id or None for identity ids): len_bits below one padded block, exactly two 2048-bit blocks, one bit and
# 31 bits into a new word; sparse ids (stored through the id -> row table), the second with 64-bit bit indices
WORLDS = [("n33", 33, None), ("n4096", 4096, None), ("n4097", 4097, None), ("n4127", 4127, None),
          ("sparse_2p20", 3000, 2**20 + 5), ("sparse_u32max", 3000, U32_MAX)]


def popcount(words):
    return int(np.bitwise_count(words).sum(dtype=np.uint64))


def bitmap_of(ids, n_bits, junk_tail=False):
    """The uint64 words of the set `ids` cut at n_bits; junk_tail: every bit of the last word at or above n_bits set too."""
    words = np.zeros((n_bits + 63) // 64, dtype=np.uint64)
    sel = np.asarray(ids, dtype=np.uint64)
    sel = sel[sel < n_bits]
    np.bitwise_or.at(words, (sel >> np.uint64(6)).astype(np.int64), np.uint64(1) << (sel & np.uint64(63)))
    if junk_tail and n_bits % 64:
        words[-1] |= np.uint64((~((1 << (n_bits % 64)) - 1)) & 0xFFFFFFFFFFFFFFFF)
    return words


def leaf_kept_of(f, n_nodes):
    """The per-node counts alone (Filter.export would also read the bitmap back: 512 MiB where id u32::MAX is stored)."""
    out = np.zeros(n_nodes, dtype=np.uint32)
    _lib.check(_lib.lib().ah_filter_export(f._handle(), None, None, out.ctypes.data_as(C.c_void_p)))
    return out


class Operand:
    def __init__(self, w, ids, f=None):
        self.ids = np.ascontiguousarray(ids, dtype=np.uint32)  # the set its bitmap holds: ascending, at most the largest id
        self.f = f if f is not None else w.index.make_filter(self.ids, sorted=True)
        self.kept = leaf_kept_of(self.f, w.n_nodes)


class World:
    def __init__(self, n, top):
        rng = np.random.default_rng(11)
        self.n, self.big = n, top == U32_MAX
        if top is None:
            ids = np.arange(n, dtype=np.uint32)
        else:  # ascending with gaps of 5 or 8: id + 3 is never stored
            ids = (np.arange(n, dtype=np.uint64) * 7 + np.arange(n, dtype=np.uint64) % 3).astype(np.uint32)
            ids[-1] = top
        self.ids = ids
        self.len_bits = int(ids[-1]) + 1
        self.vecs = rng.standard_normal((n, DIMS)).astype(np.float32)
        self.ds = Dataset(D.Euclidean, DIMS, n)
        self.ds.upload_vectors(ids, self.vecs)
        self.ds.finalize()
        self.forest = self.ds.build_forest(shard.tree_seeds(11, range(TREES)), split_after=SPLIT_AFTER)
        self.index = self.ds.create_index(self.forest)
        ex = self.index.export(normals=False)
        self.nodes, self.desc = ex["nodes"], ex["descendants"]
        self.n_nodes = self.nodes.size
        self.leaf = np.flatnonzero((self.nodes["kind"] == 1) & (self.nodes["count"] > 0))
        self.leaf_len = self.nodes["count"][self.leaf].astype(np.int64)
        # the leaves of tree 0, by a walk from its root
        stack, leaves0 = [int(ex["roots"][0])], []
        while stack:
            nd = self.nodes[stack.pop()]
            if nd["kind"] == 1:
                leaves0.append((int(nd["offset"]), int(nd["count"])))
            else:
                stack += [int(nd["left"]), int(nd["right"])]
        ids_of = lambda some: np.unique(np.concatenate([self.desc[o:o + c] for o, c in some] + [np.zeros(0, np.uint32)]))  # noqa: E731
        self.ops = {"half": Operand(self, ids[::2]), "p05": Operand(self, ids[::20]), "p002": Operand(self, ids[::500]),
                    "empty": Operand(self, np.zeros(0, np.uint32)), "all": Operand(self, ids),
                    # all ids of some leaves of tree 0: k == c and k == 0 both occur there, parts in the other trees
                    "cluster": Operand(self, ids_of(leaves0[::2])), "cluster2": Operand(self, ids_of(leaves0[1::3]))}
        if top is not None:  # ids that are not stored, through the bitmap entry point (n_bits == len_bits)
            mixed = np.union1d(ids[1::3], ids[:-1:2] + np.uint32(3)).astype(np.uint32)
            self.ops["unstored"] = Operand(self, mixed, self.index.make_filter_bitmap(bitmap_of(mixed, self.len_bits), self.len_bits))

    def numpy_ids(self, op, names):
        """The ascending id list of the expression, by numpy."""
        sets = [self.ops[x].ids for x in names]
        if op == AND:
            out = functools.reduce(np.intersect1d, sets)
        elif op == OR:
            out = functools.reduce(np.union1d, sets)
        elif op == ANDNOT:
            out = np.setdiff1d(sets[0], functools.reduce(np.union1d, sets[1:])) if len(sets) > 1 else sets[0]
        else:
            assert not self.big, "the complement is a 16 GiB list there"
            out = np.setdiff1d(np.arange(self.len_bits, dtype=np.uint32), sets[0])
        return np.ascontiguousarray(out, dtype=np.uint32)

    def predicted(self, op, names):
        """leaves, leaves_walked, ids_walked of ah_filter_combine_stats by `derive` over the operands' exported counts."""
        ks = np.stack([self.ops[x].kept[self.leaf] for x in names], axis=1)
        walk = np.array([derive(op, c, k) == WALK for c, k in zip(self.leaf_len.tolist(), ks.tolist())], dtype=bool)
        return {"leaves": int(self.leaf.size), "leaves_walked": int(walk.sum()), "ids_walked": int(self.leaf_len[walk].sum())}

    def combine(self, op, names, **tun):
        with _lib.tuning(**tun):
            return self.index.combine_filters(OP_NAME[op], [self.ops[x].f for x in names], want_stats=True)

    def same_as_list(self, got, want_ids, what, listed=None):
        """`got` is bit for bit the filter ah_filter_create makes of want_ids; returns its export.  `listed` is the popcount
        unless the caller knows better (a bitmap-made filter counts the bits it was given above the largest stored id too)."""
        with self.index.make_filter(want_ids, sorted=True) as want:
            ge, we = got.export(), want.export()
            gi, wi = got.info(), want.info()
        assert ge["len_bits"] == we["len_bits"] == self.len_bits, what
        assert np.array_equal(ge["bits"], we["bits"]), what
        assert np.array_equal(ge["leaf_kept"], we["leaf_kept"]), what
        assert gi["stored"] == wi["stored"], (what, gi, wi)
        assert gi["listed"] == (popcount(ge["bits"]) if listed is None else listed), (what, gi)
        return ge

    def close(self):
        self.index.close()  # (closes its filters first)
        self.forest.close()
        self.ds.close()


@pytest.fixture(scope="module", params=WORLDS, ids=[w[0] for w in WORLDS])
def world(request):
    _name, n, top = request.param
    w = World(n, top)
    yield w
    w.close()


def operand_tuples(w, op):
    if op == NOT:
        if w.big:  # (two 512 MiB exports per operand there)
            return [("half",), ("p05",), ("empty",), ("cluster",)]
        names = ["half", "p05", "p002", "empty", "all", "cluster"] + (["unstored"] if "unstored" in w.ops else [])
        return [(x,) for x in names]
    if w.big:  # every export is 512 MiB there: one expression of every size, the clustered operands among them
        return [("half",), ("cluster", "unstored"), ("cluster", "cluster2", "half")]
    out = [("half",), ("half", "p05"), ("cluster", "cluster2"), ("cluster", "half"), ("empty", "half"), ("half", "empty"),
           ("all", "p002"), ("half", "all"), ("half", "p05", "cluster"), ("cluster", "cluster2", "all"), ("p002", "empty", "cluster")]
    if "unstored" in w.ops:
        out += [("unstored", "half"), ("cluster", "unstored", "p05")]
    return out


@pytest.mark.parametrize("op", [AND, OR, ANDNOT], ids=["and", "or", "andnot"])
def test_expressions_equal_the_list_made_filter(world, op):
    w = world
    total_ids = int(w.leaf_len.sum())
    for k, names in enumerate(operand_tuples(w, op)):
        what = (OP_NAME[op], names)
        got, st = w.combine(op, names)
        ge = w.same_as_list(got, w.numpy_ids(op, names), what)
        # the schedule: what was derived and what was walked is what the rules say, from the operands' own counts
        want_st = w.predicted(op, names)
        assert {x: st[x] for x in want_st} == want_st, (what, st)
        assert st["words"] * 32 >= w.len_bits and st["words"] % 64 == 0, st
        if len(names) == 1:
            assert st["leaves_walked"] == 0, (what, st)
        if names[:2] == ("cluster", "cluster2") and len(w.leaf) > 8:  # the leaves of tree 0 at the least are settled by the counts
            assert st["leaves_walked"] < st["leaves"] and st["ids_walked"] < total_ids, (what, st)
        # the derivation off: every leaf walked, the same filter
        if not w.big or k == 1:
            got0, st0 = w.combine(op, names, AH_FILTER_COMBINE_SHORTCUT=0)
            g0 = got0.export()
            assert np.array_equal(g0["bits"], ge["bits"]) and np.array_equal(g0["leaf_kept"], ge["leaf_kept"]), what
            i0, i1 = got0.info(), got.info()  # (device_bytes is what the allocator handed out: a recycled block may be larger)
            assert (i0["listed"], i0["stored"]) == (i1["listed"], i1["stored"]), (what, i0, i1)
            assert st0["leaves_walked"] == st0["leaves"] == w.leaf.size and st0["ids_walked"] == total_ids, (what, st0)
            got0.close()
        got.close()


def test_not_masks_the_tail_and_counts_past_2_to_the_32(world):
    w = world
    words = (w.len_bits + 31) // 32
    tail_mask = 0xFFFFFFFF if w.len_bits % 32 == 0 else (1 << (w.len_bits % 32)) - 1
    kept_len = np.zeros(w.n_nodes, dtype=np.int64)
    kept_len[w.leaf] = w.leaf_len
    for (name,) in operand_tuples(w, NOT):
        a = w.ops[name]
        for shortcut in (1, 0):
            if w.big and (shortcut == 0) != (name == "cluster"):
                continue  # (one 512 MiB export per operand there)
            got, st = w.combine(NOT, (name,), AH_FILTER_COMBINE_SHORTCUT=shortcut)
            info = got.info()
            if not w.big:
                ge = w.same_as_list(got, w.numpy_ids(NOT, (name,)), ("not", name, shortcut))
            else:  # no list of 2^32 - |a| ids: numpy's complement of the operand's own words (module docstring)
                ge = got.export()
                assert ge["len_bits"] == 2**32 and np.array_equal(ge["bits"], ~a.f.export()["bits"]), name
                assert np.array_equal(ge["leaf_kept"].astype(np.int64), kept_len - a.kept.astype(np.int64)), name
                assert info["stored"] == w.n - a.f.info()["stored"], (name, info)
            assert info["listed"] == w.len_bits - a.ids.size == popcount(ge["bits"]), (name, info)  # (2^32 for the empty operand)
            assert ge["bits"].size == words and int(ge["bits"][-1]) & ~tail_mask == 0, name
            want = {"leaves": int(w.leaf.size), "leaves_walked": 0 if shortcut else int(w.leaf.size),
                    "ids_walked": 0 if shortcut else int(w.leaf_len.sum())}
            assert {x: st[x] for x in want} == want, (name, shortcut, st)
            if shortcut and name in (("empty",) if w.big else ("half", "empty")):
                # NOT NOT a == a: no bit beyond len_bits came back, neither in the last word nor in the padding words, which
                # the second pass reads and counts (listed) like the others
                back = ~got
                be = back.export()
                ae = a.f.export()
                assert np.array_equal(be["bits"], ae["bits"]) and np.array_equal(be["leaf_kept"], ae["leaf_kept"]), name
                assert back.info()["listed"] == a.ids.size and back.info()["stored"] == a.f.info()["stored"], name
                back.close()
            if shortcut and name == "p05":  # (NOT a) AND b has a list on every world
                both = got & w.ops["half"].f
                w.same_as_list(both, np.setdiff1d(w.ops["half"].ids, a.ids).astype(np.uint32), ("not-and", name))
                both.close()
            got.close()
    if w.big:
        assert w.len_bits - w.ops["empty"].ids.size == 2**32  # the `listed` asserted above did not fit in 32 bits


def test_repeated_operands_64_operands_and_combined_operands(world):
    w = world
    a, b, c = w.ops["half"], w.ops["p05"], w.ops["cluster"]
    empty = np.zeros(0, np.uint32)
    for op, want in ((AND, a.ids), (OR, a.ids), (ANDNOT, empty)):
        got, st = w.combine(op, ("half", "half"))
        w.same_as_list(got, want, (OP_NAME[op], "a a"))
        assert {x: st[x] for x in ("leaves", "leaves_walked", "ids_walked")} == w.predicted(op, ("half", "half")), st
        got.close()
    # a combine of combined filters, through the operators: (a & c) | (b - c), then minus NOT a
    ac, bc = a.f & c.f, b.f - c.f
    both = ac | bc
    want = np.union1d(np.intersect1d(a.ids, c.ids), np.setdiff1d(b.ids, c.ids)).astype(np.uint32)
    w.same_as_list(both, want, "nested")
    na = ~a.f
    last = both - na
    w.same_as_list(last, np.intersect1d(want, a.ids).astype(np.uint32), "nested minus not")
    assert all(f in w.index._filters for f in (ac, bc, both, na, last))  # registered like any other filter
    for f in (ac, bc, both, na, last):
        f.close()
    if w.big:
        return  # (64 more operands of 512 MiB each add nothing there)
    # 64 operands at once: OR of 64 disjoint lists, and a list minus 63 of them
    parts = [Operand(w, w.ids[i::67]) for i in range(_lib.FILTER_COMBINE_MAX)]
    try:
        pos = np.arange(w.n)
        got, st = w.index.combine_filters("or", [p.f for p in parts], want_stats=True)
        w.same_as_list(got, w.ids[pos % 67 < 64], "or of 64")
        assert st["leaves"] == w.leaf.size
        got.close()
        got = w.index.combine_filters("andnot", [w.ops["all"].f] + [p.f for p in parts[:63]])
        w.same_as_list(got, w.ids[pos % 67 >= 63], "all minus 63")
        got.close()
        got = w.index.combine_filters("and", [w.ops["all"].f] * 63 + [a.f])
        w.same_as_list(got, a.ids, "and of 64")
        got.close()
        with pytest.raises(_lib.ArroyHipError, match="n = 65"):
            w.index.combine_filters("or", [p.f for p in parts] + [a.f])
    finally:
        for p in parts:
            p.f.close()


def test_make_filter_bitmap_equals_the_list_of_its_set_bits(world):
    w = world
    # candidates: stored ids, and on sparse worlds ids that are not stored; ids above the largest stored one where there are any
    base = np.union1d(w.ids[::3], w.ids[:-1:5] + np.uint32(3 if "unstored" in w.ops else 0)).astype(np.uint64)
    above = w.len_bits + np.array([0, 1, 37, 64, 200], dtype=np.uint64)
    cases = [("below", w.len_bits - min(w.len_bits - 1, 21), False), ("below, junk in the tail", max(1, w.len_bits - 5), True),
             ("equal", w.len_bits, False), ("small", min(w.len_bits, 70), True), ("none", 0, False)]
    if not w.big:  # (2^32 + 201 bits: nothing new after `equal`)
        cases += [("above", w.len_bits + 201, False), ("above, junk in the tail", w.len_bits + 190, True)]
    for what, n_bits, junk in cases:
        if w.big and n_bits > 2**20 and what != "equal":
            continue  # one 512 MiB upload on that world
        ids = np.concatenate([base, above])
        ids = ids[ids < n_bits]
        got = w.index.make_filter_bitmap(bitmap_of(ids, n_bits, junk_tail=junk), n_bits)
        lst = ids.astype(np.uint32)
        w.same_as_list(got, lst, what, listed=lst.size)
        with w.index.make_filter(lst, sorted=True) as want:
            gi, wi = got.info(), want.info()  # `listed` too: the bits above len_bits count
            assert (gi["listed"], gi["stored"]) == (wi["listed"], wi["stored"]) == (lst.size, np.isin(lst, w.ids).sum()), (what, gi, wi)
        got.close()
    with pytest.raises(ValueError):
        w.index.make_filter_bitmap(np.zeros(1, np.uint64), 65)


def search_world():
    for name, n, top in WORLDS:
        if name == "n4097":
            return World(n, top)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_searches_under_a_combined_filter_equal_those_under_the_list():
    w = search_world()
    try:
        rng = np.random.default_rng(5)
        queries = (w.vecs[rng.choice(w.n, 40, replace=False)] + rng.standard_normal((40, DIMS)).astype(np.float32) * np.float32(0.1)).astype(np.float32)
        pairs = []  # (combined, list-made) filters of the same sets: a share near 0.5, one below the wave descent's 5 %
        for op, names in ((OR, ("half", "cluster")), (AND, ("half", "p05")), (ANDNOT, ("all", "half", "cluster2"))):
            pairs.append((w.combine(op, names)[0], w.index.make_filter(w.numpy_ids(op, names), sorted=True)))
        for comb, lst in pairs:
            res = []
            for f in (comb, lst):
                w.index.stats(reset=True)
                res.append(([w.index.search(10, queries=queries[i:i + 1], search_k=200, raw=True, candidates=f) for i in range(40)]
                            + [w.index.search(10, queries=queries, search_k=200, raw=True, candidates=f)], w.index.stats()))
            for x, y in zip(res[0][0], res[1][0]):
                assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(x, y))
            assert res[0][1] == res[1][1], (res[0][1], res[1][1])  # the same path choices: every counter of ah_search_stats
            assert res[0][1]["filtered_queries"] == 80 and res[0][1]["leaf_kept_passes"] == 0
        # one ah_search_batch_filters call that mixes them: every query twice, under the combined and under the list-made filter
        filters = [f for pair in pairs for f in pair]
        q2 = np.repeat(queries, 2, axis=0)
        slots = np.array([2 * (i % 3) + j for i in range(40) for j in range(2)], dtype=np.uint32)
        for gmin in (1, 16, 1000):
            with _lib.tuning(AH_SEARCH_FILTER_GROUP_MIN=gmin):
                oi, od, oc = w.index.search(10, queries=q2, search_k=200, raw=True, filters=filters, filter_of_query=slots)
            assert np.array_equal(oi[0::2], oi[1::2]) and np.array_equal(bits(od[0::2]), bits(od[1::2])) and np.array_equal(oc[0::2], oc[1::2]), gmin
            assert int(oc.sum()) > 0
    finally:
        w.close()


def test_lifecycle_counters_and_refusals():
    w = search_world()
    L = _lib.lib()
    other = None
    try:
        dev = w.ds.device
        a, b = w.ops["half"], w.ops["cluster"]
        want_ids = np.intersect1d(a.ids, b.ids).astype(np.uint32)
        w.index.combine_filters("and", [a.f, b.f]).close()  # (a first call warms the calling thread's context up)
        for make in (lambda: w.index.combine_filters("and", [a.f, b.f]),
                     lambda: w.index.make_filter_bitmap(bitmap_of(want_ids, w.len_bits), w.len_bits)):
            live0, _ = _lib.device_cache_stats(dev)
            st0 = w.index.filter_stats()
            f = make()
            live1, _ = _lib.device_cache_stats(dev)
            st1 = w.index.filter_stats()
            assert live1 - live0 == f.info()["device_bytes"] > 0, (live0, live1, f.info())
            assert st1["filters_alive"] == st0["filters_alive"] + 1 and st1["filters_created"] == st0["filters_created"] + 1
            assert st1["leaf_kept_passes"] == st0["leaf_kept_passes"] + 1
            f.close()
            assert _lib.device_cache_stats(dev)[0] == live0 and w.index.filter_stats()["filters_alive"] == st0["filters_alive"]
        # an operand of another index, named by its position; NULL among real operands
        other = Index(w.ds, w.forest)
        fo = other.make_filter(a.ids, sorted=True)
        with pytest.raises(_lib.ArroyHipError, match=r"operands\[1\] belongs to another index"):
            w.index.combine_filters("or", [a.f, fo])
        with pytest.raises(_lib.ArroyHipError, match=r"operands\[2\] belongs to another index"):
            w.index.combine_filters("andnot", [a.f, a.f, fo, b.f])
        h = C.c_void_p()
        arr = (C.c_void_p * 2)(a.f._handle(), None)
        assert L.ah_filter_combine(AND, arr, 2, C.byref(h), None) == 5 and b"operands[1] is NULL" in L.ah_last_error() and not h.value
        # destroying the operands first leaves the result usable; the index refuses to go or to be suspended under it alone
        oa, ob = other.make_filter(a.ids, sorted=True), other.make_filter(b.ids, sorted=True)
        comb = other.combine_filters("and", [oa, ob])
        for f in (fo, oa, ob):
            f.close()
        assert other.filter_stats()["filters_alive"] == 1
        assert L.ah_index_destroy(other._h) == 5 and b"live filter" in L.ah_last_error()
        assert L.ah_index_suspend(other._h) == 5 and b"live filter" in L.ah_last_error()
        q = w.vecs[:7]
        got = other.search(10, queries=q, search_k=200, raw=True, candidates=comb)
        want = w.index.search(10, queries=q, search_k=200, raw=True, candidates=want_ids, candidates_sorted=True)
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, want))
        comb.close()
        # a suspended index is refused
        other.suspend()
        with pytest.raises(_lib.ArroyHipError, match="suspended"):
            other.make_filter_bitmap(bitmap_of(want_ids, w.len_bits), w.len_bits)
        other.resume()
        other.make_filter_bitmap(bitmap_of(want_ids, w.len_bits), w.len_bits).close()
    finally:
        if other is not None:
            other.close()
        w.close()


def test_combine_and_create_bitmap_survive_every_allocation_failure():
    """The sweep of tests/test_gpu_search_filters.py: every allocation of a call fails once (the library's own injection, a
    status by design, no device fault), nothing is left behind, and the next call gives the right filter."""
    w = search_world()
    try:
        a, b = w.ops["half"], w.ops["cluster"]
        want_ids = np.union1d(a.ids, b.ids).astype(np.uint32)
        words = bitmap_of(want_ids, w.len_bits)
        for make in (lambda: w.index.combine_filters("or", [a.f, b.f]), lambda: w.index.make_filter_bitmap(words, w.len_bits)):
            make().close()
            alive = w.index.filter_stats()
            live, _ = _lib.device_cache_stats(w.ds.device)
            seen = sweep(make, cleanup=lambda f: f.close())
            assert len(seen) >= 2 and OOM in seen, seen  # the handle and the filter's block
            # a failure leaves nothing behind and moves no counter: each of the two sweeps ends with the one call that succeeds
            want_st = dict(alive, filters_created=alive["filters_created"] + 2, leaf_kept_passes=alive["leaf_kept_passes"] + 2)
            assert w.index.filter_stats() == want_st, (w.index.filter_stats(), want_st)
            assert _lib.device_cache_stats(w.ds.device)[0] == live
            f = make()
            w.same_as_list(f, want_ids, "after the sweep")
            f.close()
    finally:
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        w.close()


# ---- one block layout, one counter layout: the five ways to make a filter agree -----------------------------------------------
# (name, rows, largest id or None for identity ids, trees).  The bitmap of a block is padded to 2048 bits, and the counters of a
# call sit 8-byte aligned behind n_nodes 32-bit counts: len_bits one bit short of and one bit into a second 2048-bit span,
# identity and sparse, each with an even and an odd n_nodes.  A tree of L leaves has 2L - 1 nodes, so the parity of n_nodes is
# that of the number of trees and no item count changes it: two trees for the even worlds, three for the odd ones.
LAYOUT_WORLDS = [("id2048", 2048, None, 2), ("id2049", 2049, None, 3), ("sp4095", 600, 4095, 3), ("sp4096", 600, 4096, 2)]


def fresh(make):
    """make() on an empty allocator cache: its first block is a new one, as large as the allocator rounds what was asked for."""
    _lib.device_cache_trim()
    return make()


def test_the_five_creators_lay_out_one_filter():
    """The same id set through ah_filter_create, ah_filter_create_bitmap, ah_filter_combine (OR of two halves),
    ah_filter_create_roaring and ah_filter_suspend + ah_filter_resume_batch (another set, edited into this one): identical
    ah_filter_export (bits, per-node counts) and identical ah_filter_info.  `device_bytes` is also held against the layout itself
    (bitmap words rounded to 64, n_nodes counts, 256 bytes, as the allocator rounds a fresh block: every creator starts from an
    empty allocator cache).  One exception, as everywhere in this module: of listed ids ABOVE the largest stored id, which no
    bitmap holds, the list, the host bitmap and the Roaring blob count in `listed` what they were given, an expression and a
    resume the bits they set — so `listed` is compared across all five for the set without such ids, and held to each
    creator's own rule for the set with them."""
    parities = {five_creators_agree(*w) for w in LAYOUT_WORLDS}
    assert parities == {0, 1}, f"n_nodes of the layout worlds: parities {parities}"


def five_creators_agree(name, n, top, trees):
    """-> n_nodes % 2 of the world's index."""
    rng = np.random.default_rng(5)
    sparse = top is not None
    ids = np.arange(n, dtype=np.uint32)
    if sparse:  # ascending, id % 6 in {0, 1, 2}: id + 3 is never stored
        ids = (np.arange(n, dtype=np.uint32) * 6 + np.arange(n, dtype=np.uint32) % 3).astype(np.uint32)
        ids[-1] = top
    len_bits = int(ids[-1]) + 1
    ds = Dataset(D.Euclidean, 8, n)
    ds.upload_vectors(ids, rng.standard_normal((n, 8)).astype(np.float32))
    ds.finalize()
    forest = ds.build_forest(shard.tree_seeds(5, range(trees)), split_after=SPLIT_AFTER)
    index = ds.create_index(forest)
    try:
        n_nodes = index.export_info()["n_nodes"]
        words = ((len_bits + 31) // 32 + 63) // 64 * 64
        want_bytes = (words * 4 + n_nodes * 4 + 256 + 4095) // 4096 * 4096
        gaps = (ids[1:-1:4] + np.uint32(3)) if sparse else np.zeros(0, np.uint32)  # (in the gaps: listed, never stored)
        inside = np.union1d(np.union1d(ids[::2], ids[-1:]), gaps).astype(np.uint32)  # the largest stored id is in the set
        above = (len_bits + np.array([0, 4, 70000])).astype(np.uint32)
        other = np.union1d(ids[::3], (ids[2:-1:5] + np.uint32(3)) if sparse else ids[:0]).astype(np.uint32)  # what the resume starts from
        for what, want in (("inside", inside), ("with ids above", np.concatenate([inside, above]))):
            n_in = int(inside.size)
            made = {}
            made["list"] = fresh(lambda: index.make_filter(want, sorted=True))
            n_bits = int(want[-1]) + 1
            made["bitmap"] = fresh(lambda: index.make_filter_bitmap(bitmap_of(want, n_bits), n_bits))
            halves = [index.make_filter(want[0::2], sorted=True), index.make_filter(want[1::2], sorted=True)]
            made["or"] = fresh(lambda: index.combine_filters("or", halves))
            made["roaring"] = fresh(lambda: index.make_filter_roaring(roaring.serialize(want)))
            made["resume"] = index.make_filter(other, sorted=True)
            made["resume"].suspend()
            fresh(lambda: index.resume_filters([made["resume"]], [(np.setdiff1d(other, want), np.setdiff1d(want, other))], edits_sorted=True))
            listed_rule = {"list": want.size, "bitmap": want.size, "roaring": want.size, "or": n_in, "resume": n_in}
            ref_e, ref_i = made["list"].export(), made["list"].info()
            assert ref_e["len_bits"] == len_bits and ref_i["stored"] == int(np.isin(inside, ids).sum()), (what, ref_i)
            assert popcount(ref_e["bits"]) == n_in and ref_i["device_bytes"] == want_bytes, (what, ref_i, want_bytes)
            for how, f in made.items():
                e, i = f.export(), f.info()
                print(name, what, how, i, "n_nodes", n_nodes)
                assert e["len_bits"] == len_bits, (what, how)
                assert np.array_equal(e["bits"], ref_e["bits"]), (what, how)
                assert np.array_equal(e["leaf_kept"], ref_e["leaf_kept"]), (what, how)
                assert (i["stored"], i["device_bytes"]) == (ref_i["stored"], ref_i["device_bytes"]), (what, how, i, ref_i)
                assert i["listed"] == listed_rule[how], (what, how, i)
                if what == "inside":
                    assert i == ref_i, (how, i, ref_i)
            for f in list(made.values()) + halves:
                f.close()
        return n_nodes % 2
    finally:
        index.close()
        forest.close()
        ds.close()
