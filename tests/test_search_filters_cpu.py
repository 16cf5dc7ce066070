"""Resident candidate filters and ah_search_batch_filters, the part that needs no device: the symbols, the ctypes table, the
refusals that are judged before a device is touched, and the host's ordering / chunking rule restated in numpy (the GPU suite,
tests/test_gpu_search_filters.py, holds ah_filter_stats of real calls against the same restatement)."""
import ctypes as C

import numpy as np
import pytest

NO_FILTER = 0xFFFFFFFF
CHUNK_CAP = 4096  # queries of one sub-batch at most (search.hip: search_shape)
NEW_SYMBOLS = ("ah_filter_create", "ah_filter_info", "ah_filter_destroy", "ah_search_batch_filters", "ah_index_filter_stats")


def plan(filter_of_query, group_min, chunk=CHUNK_CAP):
    """The sub-batches of one ah_search_batch_filters call: [(kind, query indices)], kind "uniform" or "mixed".
    Query indices ordered stably by slot, unfiltered first; a run of one slot of at least `group_min` queries is cut into uniform
    sub-batches of at most `chunk`; the shorter runs are packed in that order into sub-batches of at most `chunk`, each of them
    mixed unless all its queries share one slot."""
    f = np.asarray(filter_of_query, dtype=np.uint32)
    key = (f.astype(np.int64) + 1) & 0xFFFFFFFF  # AH_NO_FILTER -> 0
    order = np.argsort(key, kind="stable")
    uniform, rest = [], []
    r0 = 0
    while r0 < order.size:
        r1 = r0 + 1
        while r1 < order.size and key[order[r1]] == key[order[r0]]:
            r1 += 1
        if r1 - r0 >= max(1, group_min):
            uniform += [("uniform", order[c:min(r1, c + chunk)]) for c in range(r0, r1, chunk)]
        else:
            rest += list(order[r0:r1])
        r0 = r1
    rest = np.asarray(rest, dtype=np.int64)
    tail = []
    for c in range(0, rest.size, chunk):
        part = rest[c:c + chunk]
        tail.append(("uniform" if np.unique(key[part]).size == 1 else "mixed", part))
    return uniform + tail


def check_plan(f, group_min):
    f = np.asarray(f, dtype=np.uint32)
    batches = plan(f, group_min)
    seen = np.concatenate([b for _k, b in batches]) if batches else np.zeros(0, np.int64)
    assert sorted(seen.tolist()) == list(range(f.size)), "every query exactly once"
    for kind, b in batches:
        assert 0 < b.size <= CHUNK_CAP
        keys = (f[b].astype(np.int64) + 1) & 0xFFFFFFFF
        # inside a sub-batch: by slot, unfiltered first, and the caller's order inside a slot
        assert (np.diff(keys) >= 0).all()
        assert all((np.diff(b[keys == k]) > 0).all() for k in np.unique(keys))
        assert (np.unique(keys).size == 1) == (kind == "uniform")
    return batches


def test_new_symbols_are_exported_and_declared():
    from arroy_amd import _lib
    L = _lib.lib()
    assert L.ah_abi_version() == 7
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert _lib.NO_FILTER == NO_FILTER
    assert C.sizeof(_lib.AhFilterStats) == 8 * 8
    assert _lib.tuning_get("AH_SEARCH_FILTER_GROUP_MIN")[0] >= 1


def test_plan_all_unfiltered_and_one_filter():
    for nq in (1, 5, 700):
        for gmin in (1, 16, 1000):
            assert [k for k, _ in check_plan(np.full(nq, NO_FILTER), gmin)] == ["uniform"]
            assert [k for k, _ in check_plan(np.zeros(nq), gmin)] == ["uniform"]


def test_plan_every_query_its_own_filter():
    b = check_plan(np.arange(100), 2)
    assert [k for k, _ in b] == ["mixed"] and b[0][1].tolist() == list(range(100))
    assert [k for k, _ in check_plan(np.arange(100), 1)] == ["uniform"] * 100
    assert [k for k, _ in check_plan(np.arange(1), 5)] == ["uniform"]


def test_plan_group_sizes_at_the_minimum_and_one_below():
    gmin = 8
    f = np.array([0] * gmin + [1] * (gmin - 1) + [NO_FILTER] * (gmin - 1) + [2] * gmin)
    rng = np.random.default_rng(3)
    f = f[rng.permutation(f.size)]
    b = check_plan(f, gmin)
    assert [k for k, _ in b] == ["uniform", "uniform", "mixed"]
    assert sorted(int(f[x[0]]) for k, x in b if k == "uniform") == [0, 2]
    assert all(x.size == gmin for k, x in b if k == "uniform")
    mixed = b[2][1]
    assert mixed.size == 2 * (gmin - 1) and (f[mixed[:gmin - 1]] == NO_FILTER).all() and (f[mixed[gmin - 1:]] == 1).all()
    # one more query of slot 1 lifts its run to the minimum: what is left over shares one slot (none) and is uniform
    b = check_plan(np.append(f, 1), gmin)
    assert [k for k, _ in b] == ["uniform"] * 4


def test_plan_above_the_chunk_cap():
    rng = np.random.default_rng(4)
    nq = 2 * CHUNK_CAP + 905
    b = check_plan(np.zeros(nq), 16)
    assert [x.size for _k, x in b] == [CHUNK_CAP, CHUNK_CAP, 905]
    f = rng.integers(0, 3000, nq)  # runs of a few queries each: all left over, cut at the cap
    b = check_plan(f, 16)
    assert [k for k, _ in b] == ["mixed"] * 3 and [x.size for _k, x in b] == [CHUNK_CAP, CHUNK_CAP, 905]
    f = np.where(rng.random(nq) < 0.6, 7, f)  # one long run beside them
    b = check_plan(f, 16)
    n7 = int((f == 7).sum())
    assert [x.size for k, x in b if k == "uniform"] == [CHUNK_CAP] * (n7 // CHUNK_CAP) + [n7 % CHUNK_CAP]
    assert sum(x.size for k, x in b if k == "mixed") == nq - n7


def test_refusals_that_need_no_device():
    from arroy_amd import _lib
    L = _lib.lib()
    q = np.zeros((2, 8), np.float32)
    oi, od, oc = np.zeros((2, 3), np.uint32), np.zeros((2, 3), np.float32), np.zeros(2, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    none = C.POINTER(C.c_void_p)()

    def refused(status, word):
        assert status == 5, status  # AH_ERR_INVALID_ARGUMENT
        assert word in L.ah_last_error().decode(), L.ah_last_error()

    # a NULL index, NULL outputs, both or neither of queries / query_items
    refused(L.ah_search_batch_filters(None, p(q), None, 2, 3, 0, 0, none, 0, None, p(oi), p(od), p(oc)), "index is NULL")
    refused(L.ah_search_batch_filters(None, p(q), None, 2, 3, 0, 0, none, 0, None, None, p(od), p(oc)), "NULL output")
    refused(L.ah_search_batch_filters(None, None, None, 2, 3, 0, 0, none, 0, None, p(oi), p(od), p(oc)), "exactly one")
    # filters NULL with a count; several filters without filter_of_query
    refused(L.ah_search_batch_filters(None, p(q), None, 2, 3, 0, 0, none, 2, None, p(oi), p(od), p(oc)), "filters is NULL")
    two = (C.c_void_p * 2)(None, None)
    refused(L.ah_search_batch_filters(None, p(q), None, 2, 3, 0, 0, two, 2, None, p(oi), p(od), p(oc)), "filter_of_query is NULL")
    # a slot that names no filter (AH_NO_FILTER itself is fine: the call then gets as far as the NULL index)
    for slots, n_filters, word in (([0, NO_FILTER], 0, "names no filter"), ([NO_FILTER, 2], 2, "names no filter"),
                                   ([NO_FILTER, NO_FILTER], 0, "index is NULL")):
        foq = np.array(slots, np.uint32)
        refused(L.ah_search_batch_filters(None, p(q), None, 2, 3, 0, 0, two, n_filters, p(foq), p(oi), p(od), p(oc)), word)
    # ah_filter_create: NULL out, NULL list with a count, an unsorted list, a duplicate id, a NULL index
    h = C.c_void_p()
    ids = np.array([1, 5, 9], np.uint32)
    refused(L.ah_filter_create(None, p(ids), 3, None), "out is NULL")
    refused(L.ah_filter_create(None, None, 3, C.byref(h)), "sorted_ids is NULL")
    refused(L.ah_filter_create(None, p(np.array([1, 9, 5], np.uint32)), 3, C.byref(h)), "strictly ascending")
    refused(L.ah_filter_create(None, p(np.array([1, 5, 5], np.uint32)), 3, C.byref(h)), "strictly ascending")
    refused(L.ah_filter_create(None, p(ids), 3, C.byref(h)), "index is NULL")
    assert not h.value
    refused(L.ah_filter_info(None, None, None, None), "filter is NULL")
    refused(L.ah_index_filter_stats(None, C.byref(_lib.AhFilterStats()), 0), "NULL argument")
    assert L.ah_filter_destroy(None) == 0
    with pytest.raises(_lib.ArroyHipError):
        _lib.check(L.ah_filter_info(None, None, None, None))
