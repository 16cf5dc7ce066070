"""Filters from serialized RoaringBitmaps: ah_filter_create_roaring / ah_filter_create_roaring_batch.

The yardstick everywhere is the existing path: ah_filter_create of roaring.deserialize(blob) (arroy_amd/roaring.py, the plain
restatement of the format), compared through Filter.export() (length, bitmap words, per-node counts) and info() (listed,
stored), for both cookie forms.  Two worlds of 16 dimensions and 3 trees:
  A  identity ids, 70 000 items: len_bits 70 000 is no multiple of 32, so the second 64Ki span is cut inside a word
  B  3 000 rows on sparse ids in [0, 200 000), the largest 199 999: `stored` goes through the dataset's id array"""
import ctypes as C
import struct

import numpy as np
import pytest

from arroy_amd import Dataset, _lib, roaring, shard
from arroy_amd import distances as D
from test_filter_roaring_cpu import EMPTY, EXAMPLE, u32
from test_gpu_search_filters import OOM, sweep_once

pytestmark = pytest.mark.gpu

DIMS, TREES, SPLIT_AFTER = 16, 3, 24
SEEDS = shard.tree_seeds(31, range(TREES))
SPAN = 1 << 16
GROUP = _lib.FILTER_RESUME_GROUP


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def vectors(ids):
    ids = np.asarray(ids, dtype=np.int64)
    return (np.sin(ids[:, None] * np.arange(1, DIMS + 1)[None, :] * 0.37) + ((ids[:, None] * 7 + np.arange(DIMS)[None, :]) % 11) * 0.1).astype(np.float32)


class World:
    def __init__(self, ids):
        self.ids = u32(ids)
        self.ds = Dataset(D.Euclidean, DIMS, self.ids.size)
        self.ds.upload_vectors(self.ids, vectors(self.ids))
        self.ds.finalize()
        self.forest = self.ds.build_forest(SEEDS, split_after=SPLIT_AFTER)
        self.index = self.ds.create_index(self.forest)
        self.len_bits = int(self.ids[-1]) + 1
        self.max_key = (self.len_bits - 1) >> 16
        ex = self.index.export(normals=False)
        leaf = (ex["nodes"]["kind"] == 1) & (ex["nodes"]["count"] > 0)
        self.leaves, self.leaf_ids = int(leaf.sum()), int(ex["nodes"]["count"][leaf].sum())

    def same_as_list(self, got, blob, what):
        """`got` is bit for bit the filter ah_filter_create makes of the ids the blob holds."""
        ids = roaring.deserialize(blob)
        with self.index.make_filter(ids, sorted=True) as want:
            ge, we = got.export(), want.export()
            gi, wi = got.info(), want.info()
        assert ge["len_bits"] == we["len_bits"] == self.len_bits, (what, ge["len_bits"], we["len_bits"])
        assert np.array_equal(ge["bits"], we["bits"]), (what, np.flatnonzero(ge["bits"] != we["bits"])[:8])
        assert np.array_equal(ge["leaf_kept"], we["leaf_kept"]), what
        assert (gi["listed"], gi["stored"]) == (wi["listed"], wi["stored"]) == (ids.size, np.intersect1d(ids, self.ids).size), (what, gi, wi)

    def expected_stats(self, conts_per_blob):
        """ah_filter_roaring_stats' container counters from what roaring.py wrote: [(key, kind, cardinality, body)] per blob."""
        want = dict(array_containers=0, bitmap_containers=0, run_containers=0, skipped_containers=0, bytes_uploaded=0)
        for conts in conts_per_blob:
            for key, kind, _, body in conts:
                if key > self.max_key:
                    want["skipped_containers"] += 1
                else:
                    want[("array_containers", "bitmap_containers", "run_containers")[kind]] += 1
                    want["bytes_uploaded"] += len(body)
        return want

    def close(self):
        self.index.close()
        self.forest.close()
        self.ds.close()


@pytest.fixture(scope="module")
def world_a():
    w = World(range(70_000))
    yield w
    w.close()


@pytest.fixture(scope="module")
def world_b():
    rng = np.random.default_rng(8)
    w = World(np.concatenate([rng.choice(199_999, 2999, replace=False), [199_999]]))
    yield w
    w.close()


@pytest.fixture(params=["identity", "sparse"])
def world(request, world_a, world_b):
    return world_a if request.param == "identity" else world_b


def hand_made(w):
    """name -> [(key, kind, cardinality, body)]: well-formed containers roaring.serialize would not write (runs it would merge,
    or containers it would store as arrays), on the last span of the world, which len_bits cuts, and on span 0."""
    k = w.max_key
    return {
        "runs_at_word_edges": [(0, roaring.RUN, 4, roaring.run_body([0, 31, 65535], [0, 1, 0]))],
        "adjacent_runs": [(0, roaring.RUN, 130, roaring.run_body([10, 64, 96, 100], [53, 31, 3, 39]))],  # 10..63 | 64..95 | 96..99 | 100..139
        "one_run_whole_span": [(k, roaring.RUN, SPAN, roaring.run_body([0], [SPAN - 1]))],
        "run_inside_one_word": [(k, roaring.RUN, 3, roaring.run_body([33], [2]))],
        "no_runs_next_to_an_array": [(0, roaring.ARRAY, 2, roaring.array_body([7, 9])), (k, roaring.RUN, 2, roaring.run_body([5, 9], [0, 0]))],
    }


def cases(w):
    """name -> ascending ids"""
    rng = np.random.default_rng(5)
    cut, base = w.len_bits, w.max_key * SPAN  # the last span: ids from `base`, stored ones below `cut`
    above = [cut, cut + 1, base + SPAN - 1]   # on the last span, above the largest stored id
    return {
        "empty": [],
        "one_id": [int(w.ids[3])],
        "largest_stored_id": [cut - 1],
        "first_id_above": [cut],
        "array_4096": rng.choice(SPAN, 4096, replace=False),
        "bitmap_4097": rng.choice(SPAN, 4097, replace=False),
        "bitmap_65536": np.arange(SPAN),
        "word_edges": [0, 31, 32, 63, 64, SPAN - 1],
        "wholly_above": [(w.max_key + 1) * SPAN + 5, (w.max_key + 2) * SPAN, 0xFFFFFFFF],
        "array_straddles": list(rng.choice(np.arange(base, cut), 40, replace=False)) + above,
        "bitmap_straddles": list(base + rng.choice(SPAN, 5000, replace=False)) + [cut - 1] + above,
        "run_straddles": list(range(base + 100, base + SPAN - 50)) + [(w.max_key + 1) * SPAN + 1],
        "three_keys": [1, 2, 3] + list(range(base + 5, base + 40)) + [(w.max_key + 3) * SPAN + 7],
        "four_keys": [9] + list(range(base, base + 300)) + [(w.max_key + 1) * SPAN + 9, (w.max_key + 5) * SPAN],
        "nine_keys": [key * SPAN + j for key in range(9) for j in range(key, 60 + key)],
        "everything_stored": w.ids,
    }


def test_every_container_kind_equals_the_list_made_filter(world):
    w = world
    blobs, names, conts = [], [], []
    for name, ids in cases(w).items():
        ids = u32(ids)
        for runs in (False, True):
            conts.append(roaring.containers(ids, runs))
            blobs.append(roaring.assemble(conts[-1], runs))
            names.append((name, runs))
    for name, cs in hand_made(w).items():
        conts.append(cs)
        blobs.append(roaring.assemble(cs, True))
        names.append((name, "by hand"))
    # the kinds and header shapes the cases are there for
    kind_of = {n: roaring.kinds(b) for n, b in zip(names, blobs)}
    assert kind_of[("array_4096", False)] == {0: roaring.ARRAY} and kind_of[("bitmap_4097", True)] == {0: roaring.BITMAP}
    assert kind_of[("bitmap_65536", False)] == {0: roaring.BITMAP} and kind_of[("bitmap_65536", True)] == {0: roaring.RUN}
    assert kind_of[("array_straddles", True)][w.max_key] == roaring.ARRAY and kind_of[("bitmap_straddles", True)][w.max_key] == roaring.BITMAP
    assert kind_of[("run_straddles", True)][w.max_key] == roaring.RUN
    assert [len(kind_of[(n, True)]) for n in ("three_keys", "four_keys", "nine_keys")] == [3, 4, 9]
    st0 = w.index.filter_stats()
    filters, st = w.index.make_filters_roaring(blobs)
    try:
        n = len(blobs)
        n_groups = (n + GROUP - 1) // GROUP
        assert (st["filters"], st["groups"], st["leaves"], st["ids_walked"]) == (n, n_groups, w.leaves, n_groups * w.leaf_ids), st
        assert {k: st[k] for k in w.expected_stats(conts)} == w.expected_stats(conts), st
        assert st["skipped_containers"] >= 6 and min(st["array_containers"], st["bitmap_containers"], st["run_containers"]) >= 4, st
        st1 = w.index.filter_stats()
        assert [st1[k] - st0[k] for k in ("filters_created", "filters_alive", "leaf_kept_passes")] == [n, n, n_groups]
        for f, blob, name in zip(filters, blobs, names):
            w.same_as_list(f, blob, name)
    finally:
        for f in filters:
            f.close()
    # the single call is the batch of one: a few of them alone, from bytes, a bytearray and a memoryview
    for i, wrap in ((names.index(("run_straddles", True)), bytes), (names.index(("bitmap_straddles", False)), bytearray),
                    (names.index(("nine_keys", True)), memoryview), (names.index(("empty", True)), bytes)):
        with w.index.make_filter_roaring(wrap(blobs[i])) as f:
            w.same_as_list(f, blobs[i], ("single", names[i]))
    assert w.index.filter_stats()["filters_alive"] == st0["filters_alive"]


def test_blobs_at_odd_addresses(world):
    """The 12347 header (4 + ceil(nc / 8) bytes) and a blob at any byte address make the payload positions odd: the same
    filters from copies at offsets 0 .. 3 of a buffer, nine containers (two flag bytes) and the worked example among them."""
    w = world
    c = cases(w)
    blobs = [roaring.serialize(u32(c["nine_keys"]), runs=True), roaring.serialize(u32(c["bitmap_straddles"])), EXAMPLE,
             roaring.serialize(u32(c["array_straddles"]), runs=True), roaring.serialize(u32(c["run_straddles"]), runs=True)]
    views = []
    for shift in range(4):
        for b in blobs:
            buf = np.zeros(len(b) + shift, dtype=np.uint8)
            buf[shift:] = np.frombuffer(b, dtype=np.uint8)
            views.append(buf[shift:])
    assert {v.ctypes.data % 2 for v in views} == {0, 1}
    filters, st = w.index.make_filters_roaring(views)
    try:
        assert st["groups"] == 2
        for f, b in zip(filters, blobs * 4):
            w.same_as_list(f, b, "odd address")
    finally:
        for f in filters:
            f.close()


@pytest.mark.parametrize("n,groups", [(1, 1), (GROUP, 1), (GROUP + 1, 2), (2 * GROUP + 1, 3)])
def test_batch_sizes_and_counters(world_b, n, groups):
    """1, G, G + 1 and 2G + 1 blobs in one call, repeated and empty ones among them: `groups` passes, ah_filter_stats moves by
    exactly (n, n, groups), the container counters are what roaring.py wrote."""
    w = world_b
    rng = np.random.default_rng(n)
    sets = []
    for i in range(n):
        if i % 5 == 1:
            ids = []
        elif i % 5 == 3 and i > 3:
            ids = sets[i - 3]  # a repeated blob
        else:
            ids = rng.choice(260_000, int(rng.integers(1, 9000)), replace=False)
        sets.append(u32(ids))
    if n == 1:
        sets = [u32(rng.choice(260_000, 7000, replace=False))]
    runs = [bool(i % 2) for i in range(n)]
    conts = [roaring.containers(s, r) for s, r in zip(sets, runs)]
    blobs = [roaring.assemble(c, r) for c, r in zip(conts, runs)]
    st0 = w.index.filter_stats()
    filters, st = w.index.make_filters_roaring(blobs)
    try:
        assert (st["filters"], st["groups"], st["leaves"], st["ids_walked"]) == (n, groups, w.leaves, groups * w.leaf_ids), st
        assert {k: st[k] for k in w.expected_stats(conts)} == w.expected_stats(conts), st
        st1 = w.index.filter_stats()
        assert [st1[k] - st0[k] for k in ("filters_created", "filters_alive", "leaf_kept_passes")] == [n, n, groups]
        assert len({f._handle() for f in filters}) == n  # independent filters, the repeated blobs too
        for i, (f, b) in enumerate(zip(filters, blobs)):
            w.same_as_list(f, b, (n, i))
        # they behave like any other filter: expressions, kept_total, suspend / resume
        if n > 1:
            both = filters[0] | filters[2]
            with w.index.make_filter(np.union1d(sets[0], sets[2]).astype(np.uint32), sorted=True) as want:
                assert np.array_equal(both.export()["bits"], want.export()["bits"]) and both.info()["stored"] == want.info()["stored"]
                assert filters[0].kept_total() == int(filters[0].export()["leaf_kept"].sum())
            both.close()
            before, stored = filters[0].export(), filters[0].info()["stored"]
            filters[0].suspend()
            w.index.resume_filters([filters[0]])
            after = filters[0].export()  # (a resumed filter's `listed` is its set bits: the ids above len_bits are gone)
            assert np.array_equal(after["bits"], before["bits"]) and np.array_equal(after["leaf_kept"], before["leaf_kept"])
            assert filters[0].info()["stored"] == stored and filters[0].info()["listed"] == int(np.bitwise_count(after["bits"]).sum())
    finally:
        for f in filters:
            f.close()
    assert w.index.filter_stats()["filters_alive"] == st0["filters_alive"]


def test_a_pass_per_filter_where_grouped_passes_are_switched_off(world_a):
    """AH_FILTER_RESUME_MIXED_MB = 0 (no room for a group's bitmaps side by side): `groups` is `filters`, the filters are the same."""
    w = world_a
    c = cases(w)
    blobs = [roaring.serialize(u32(c[k]), runs=r) for k, r in (("bitmap_straddles", False), ("run_straddles", True), ("empty", False))]
    st0 = w.index.filter_stats()
    with _lib.tuning(AH_FILTER_RESUME_MIXED_MB=0):
        filters, st = w.index.make_filters_roaring(blobs)
    try:
        assert (st["filters"], st["groups"], st["ids_walked"]) == (3, 3, 3 * w.leaf_ids), st
        assert w.index.filter_stats()["leaf_kept_passes"] == st0["leaf_kept_passes"] + 3
        for f, b in zip(filters, blobs):
            w.same_as_list(f, b, "a pass per filter")
    finally:
        for f in filters:
            f.close()


def test_searches_under_roaring_made_filters_equal_those_under_list_made_ones(world_a):
    w = world_a
    rng = np.random.default_rng(4)
    nq = 24
    queries = (vectors(rng.choice(70_000, nq, replace=False)) + rng.standard_normal((nq, DIMS)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    sets = [u32(range(0, 70_000, 2)), u32(rng.choice(80_000, 400, replace=False)), u32(range(60_000, 69_000)), u32(rng.choice(70_000, 30_000, replace=False))]
    blobs = [roaring.serialize(s, runs=bool(i % 2)) for i, s in enumerate(sets)]
    made, _ = w.index.make_filters_roaring(blobs)
    listed = [w.index.make_filter(s, sorted=True) for s in sets]
    try:
        slots = np.arange(nq, dtype=np.uint32) % len(sets)
        for gmin in (1, 1000):
            with _lib.tuning(AH_SEARCH_FILTER_GROUP_MIN=gmin):
                a = w.index.search(10, queries=queries, search_k=300, raw=True, filters=made, filter_of_query=slots)
                b = w.index.search(10, queries=queries, search_k=300, raw=True, filters=listed, filter_of_query=slots)
            assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)), gmin
            assert int(a[2].sum()) > 0 and all(set(a[0][q][:a[2][q]].tolist()) <= set(sets[slots[q]].tolist()) for q in range(nq))
    finally:
        for f in made + listed:
            f.close()


def test_query_builder_takes_serialized_candidates():
    """QueryBuilder.candidates(bytes): a filter made for the query and closed after it; the hits are those under the id set."""
    import random

    import arroy_amd.index as I
    dims, n = 24, 600
    vecs = np.random.default_rng(5).standard_normal((n, dims)).astype(np.float32)
    db = I.Database(D.Euclidean)
    wr = I.Writer(db, 0, dims)
    for i in range(n):
        wr.add_item(i, vecs[i])
    wr.builder(random.Random(40)).n_trees(4).build()
    reader = I.Reader.open(db, 0)
    try:
        ids = u32(range(100, 400, 3))
        for wrap in (bytes, bytearray, memoryview):
            got = reader.nns(5).search_k(200).candidates(wrap(roaring.serialize(ids, runs=True))).by_vector(vecs[150])
            want = reader.nns(5).search_k(200).candidates(ids.tolist()).by_vector(vecs[150])
            assert got == want and got and all(int(i) in set(ids.tolist()) for i, _ in got)
        assert wr._st.index.filter_stats()["filters_alive"] == 0
        with reader.make_filter_roaring(roaring.serialize(ids)) as f:
            assert f.info()["listed"] == ids.size == f.info()["stored"]
        fs, st = reader.make_filters_roaring([roaring.serialize(ids), EMPTY])
        assert st["filters"] == 2 and [f.info()["listed"] for f in fs] == [ids.size, 0]
        for f in fs:
            f.close()
    finally:
        wr._st.index.close()
        wr._st.dataset.close()


# ---- refusals found on the device ----------------------------------------------------------------------------------------------

def malformed_payloads(w):
    """name -> ([(key, kind, cardinality, body)], the container the refusal names, a word of it).  Checked input with a status
    code by design: the kernel indexes by nothing it has not bounded, so none of these touches memory outside its span."""
    k = w.max_key
    rng = np.random.default_rng(2)
    lows = np.sort(rng.choice(SPAN, 5000, replace=False))
    ok = (0, roaring.ARRAY, 3, roaring.array_body([1, 2, 3]))
    asc = np.arange(0, 600, 2)
    swapped = asc.copy()
    swapped[[255, 256]] = swapped[[256, 255]]  # across the boundary of two threads' sixteen values
    return {
        "unsorted_array": ([ok, (k, roaring.ARRAY, 300, roaring.array_body(swapped))], 1, "ascend"),
        "array_value_twice": ([(k, roaring.ARRAY, 3, roaring.array_body([4, 4, 9]))], 0, "ascend"),
        "bitmap_cardinality": ([ok, (k, roaring.BITMAP, 5001, roaring.bitmap_body(lows))], 1, "popcount"),
        "overlapping_runs": ([ok, (k, roaring.RUN, 31, roaring.run_body([10, 25], [20, 9]))], 1, "overlap"),  # 10..30 and 25..34
        "runs_out_of_order": ([(k, roaring.RUN, 4, roaring.run_body([100, 10], [1, 1]))], 0, "out of order"),
        "run_past_65535": ([(k, roaring.RUN, 20, roaring.run_body([65530], [19]))], 0, "past 65535"),
        "run_cardinality": ([ok, (k, roaring.RUN, 12, roaring.run_body([10, 40], [4, 4]))], 1, "total length"),
    }


def test_malformed_payloads_are_refused_by_name_and_leave_nothing(world):
    w = world
    L = _lib.lib()
    good = [roaring.serialize(u32(cases(w)["nine_keys"]), runs=True), roaring.serialize(u32(cases(w)["bitmap_straddles"]))]
    for f in w.index.make_filters_roaring(good)[0]:  # (a first call warms the calling thread's context up)
        f.close()
    st0 = w.index.filter_stats()
    for name, (conts, container, word) in malformed_payloads(w).items():
        blob = roaring.assemble(conts, True)
        with pytest.raises(ValueError):
            roaring.deserialize(blob)
        batch = [good[0], blob, good[1]]
        arrs = [np.frombuffer(b, dtype=np.uint8) for b in batch]
        ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * 3)(*[a.size for a in arrs])
        out = (C.c_void_p * 3)(0xDEAD, 0xDEAD, 0xDEAD)
        stats = _lib.AhFilterRoaringStats()
        status = L.ah_filter_create_roaring_batch(w.index._h, ptrs, lens, 3, out, C.byref(stats))
        text = L.ah_last_error().decode()
        assert status == 5 and f"blobs[1]: container {container}:" in text and word in text, (name, status, text)
        assert [out[i] for i in range(3)] == [None, None, None] and stats.filters == 0, name
        assert w.index.filter_stats() == st0, name
    # two malformed blobs: the lowest (blob, container) is the one reported
    bad = malformed_payloads(w)
    batch = [good[0], roaring.assemble(bad["bitmap_cardinality"][0], True), roaring.assemble(bad["unsorted_array"][0], True)]
    with pytest.raises(_lib.ArroyHipError) as e:
        w.index.make_filters_roaring(batch)
    assert e.value.status == 5 and "blobs[1]: container 1:" in str(e.value) and "popcount" in str(e.value)
    # a following valid call succeeds
    filters, st = w.index.make_filters_roaring(good)
    for f, b in zip(filters, good):
        w.same_as_list(f, b, "after the refusals")
        f.close()
    assert w.index.filter_stats()["filters_alive"] == st0["filters_alive"]


def test_refused_on_a_suspended_index_after_the_structure(world_b):
    w = world_b
    bad = struct.pack("<I", 1) + EMPTY[4:]
    w.index.suspend()
    try:
        with pytest.raises(_lib.ArroyHipError) as e:
            w.index.make_filter_roaring(EXAMPLE)
        assert e.value.status == 5 and "suspended" in str(e.value)
        with pytest.raises(_lib.ArroyHipError) as e:
            w.index.make_filters_roaring([EXAMPLE, bad])
        assert "blobs[1]:" in str(e.value) and "unknown cookie" in str(e.value)
    finally:
        w.index.resume()


# ---- every allocation failing once --------------------------------------------------------------------------------------------

def test_the_batch_call_survives_every_allocation_failure(world_b):
    """The sweep of tests/test_gpu_faults.py (the library's own injection: a status by design, no device fault).  Every failed
    attempt leaves no filter and no counter moved; the last attempt succeeds and is correct."""
    w = world_b
    n = GROUP + 1
    rng = np.random.default_rng(1)
    blobs = [roaring.serialize(u32(rng.choice(230_000, 3000 + 500 * i, replace=False)), runs=bool(i % 2)) for i in range(n)]
    for f in w.index.make_filters_roaring(blobs)[0]:  # (a first call warms the calling thread's context up: its pinned staging)
        f.close()
    alive = w.index.filter_stats()["filters_alive"]

    def create():
        st0 = w.index.filter_stats()
        try:
            return w.index.make_filters_roaring(blobs)
        except _lib.ArroyHipError:
            left = _lib.tuning_get("AH_FAIL_ALLOC_AFTER")[0]
            _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
            assert w.index.filter_stats() == st0
            _lib.tuning_set("AH_FAIL_ALLOC_AFTER", left)
            raise

    def cleanup(res):
        for i, f in enumerate(res[0]):
            w.same_as_list(f, blobs[i], ("after the sweep", i))
            f.close()
    try:
        seen = sweep_once(create, cleanup)
        held = sum(_lib.device_cache_stats(w.ds.device))
        again = sweep_once(create, cleanup)
        assert sum(_lib.device_cache_stats(w.ds.device)) == held and again == seen  # nothing leaks
        assert len(seen) >= 2 * n + 3 and OOM in seen, seen  # a handle and a block per filter, the call's buffer, host vectors
        assert w.index.filter_stats()["filters_alive"] == alive
    finally:
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
