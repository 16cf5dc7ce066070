"""Per-query count, search_k and oversampling in one batched call (ah_search_batch_params), the part that needs no device: the
symbols, the ctypes table, the refusals that are judged before a device is touched, and the host's cutting rule restated in
numpy (the GPU suite, tests/test_gpu_search_params.py, holds ah_params_stats of real calls against the same restatement)."""
import ctypes as C

import numpy as np

from test_search_filters_cpu import CHUNK_CAP, NO_FILTER
from test_search_filters_cpu import plan as filters_plan

NEW_SYMBOLS = ("ah_search_batch_params", "ah_index_params_stats")
CHUNK_BYTES = 1536 << 20  # scratch of one sub-batch at most (search.hip: kSearchChunkBytes)
SORT_LDS = 16384          # candidate ids sorted in LDS per query; a longer buffer is padded to a power of two (search.hip: kSortLds)
BATCH_TOPK_MAX = 2048     # the largest count of the batched top-k (batch.hip: batch_supported)
KEY_CHUNK = 4096          # keys per LDS sort of the top-k kernels (batch.hip / distance.hip: kChunk)


def next_pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def extent(count, search_k, oversampling, n_trees, desc_len, max_desc, default_oversampling=1):
    """(effective search_k, stride of the candidate buffer) of one query (search.hip: search_extent)."""
    sk = int(search_k) if search_k else int(count) * n_trees
    sk *= int(oversampling) if oversampling else default_oversampling
    sk = min(sk, desc_len)
    stride = min(sk + max_desc, desc_len)
    if stride > SORT_LDS:
        stride = max(2, next_pow2(stride))
    return sk, stride


def query_bytes(stride, count, row_bytes):
    """Scratch one query costs in a sub-batch whose largest stride and count are these (search.hip: search_query_bytes)."""
    stride, count = int(stride), int(count)
    if count <= BATCH_TOPK_MAX:
        key_bytes = 2 * ((stride + KEY_CHUNK - 1) // KEY_CHUNK) * KEY_CHUNK * 8
    elif min(count, stride) > KEY_CHUNK // 2:
        key_bytes = next_pow2(stride) * 8 + 64 + 64
    else:
        key_bytes = ((stride + KEY_CHUNK - 1) // KEY_CHUNK) * KEY_CHUNK * 16 + 64 + 64
    return stride * 8 + key_bytes + count * 8 + row_bytes + 4096


def plan(params_stride, counts, filter_of_query, group_min, sort, row_bytes=0):
    """The sub-batches of one ah_search_batch_params call: [(kind, query indices)], kind "uniform" or "mixed".
    Query indices ordered stably by (slot, unfiltered first; count beyond the batched top-k last; with `sort` the stride of the
    candidate buffer).  A run of one (slot, big) of at least `group_min` queries is cut into uniform sub-batches; the shorter
    runs are packed in that order — those of batched counts, then those of big counts — into sub-batches, each of them mixed
    unless all its queries share one slot.  Every sub-batch grows while it holds at most CHUNK_CAP queries and as many times
    query_bytes(its largest stride, its largest count) stay within CHUNK_BYTES.  (Which sub-batches are varied: stats_of.)"""
    stride = np.asarray(params_stride, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    f = np.asarray(filter_of_query, dtype=np.uint32)
    slot_key = (f.astype(np.int64) + 1) & 0xFFFFFFFF  # AH_NO_FILTER -> 0
    run_key = slot_key * 2 + (counts > BATCH_TOPK_MAX)
    order = np.lexsort((np.arange(f.size), stride if sort else np.zeros_like(stride), run_key))

    def cut(idx, may_mix):
        out, c0 = [], 0
        while c0 < len(idx):
            c1, st, cn = c0, 0, 0
            while c1 < len(idx) and c1 - c0 < CHUNK_CAP:
                ns, nc = max(st, int(stride[idx[c1]])), max(cn, int(counts[idx[c1]]))
                if c1 > c0 and (c1 - c0 + 1) * query_bytes(ns, nc, row_bytes) > CHUNK_BYTES:
                    break
                st, cn, c1 = ns, nc, c1 + 1
            part = np.asarray(idx[c0:c1], dtype=np.int64)
            out.append(("mixed" if may_mix and np.unique(slot_key[part]).size > 1 else "uniform", part))
            c0 = c1
        return out

    uniform, rest = [], ([], [])
    r0 = 0
    while r0 < order.size:
        r1 = r0 + 1
        while r1 < order.size and run_key[order[r1]] == run_key[order[r0]]:
            r1 += 1
        if r1 - r0 >= max(1, group_min):
            uniform += cut(order[r0:r1], False)
        else:
            rest[int(run_key[order[r0]] & 1)].extend(order[r0:r1].tolist())
        r0 = r1
    return uniform + cut(rest[0], True) + cut(rest[1], True)


def stats_of(batches, counts, search_ks):
    """ah_params_stats of one call that was cut into `batches`."""
    counts, search_ks = np.asarray(counts, dtype=np.int64), np.asarray(search_ks, dtype=np.int64)
    varied = [b for _k, b in batches if np.unique(counts[b]).size > 1 or np.unique(search_ks[b]).size > 1]
    return {"calls": 1, "batches": len(batches), "varied_batches": len(varied), "queries": int(sum(b.size for _k, b in batches)),
            "varied_queries": int(sum(b.size for b in varied)),
            "big_count_queries": int(sum(b.size for _k, b in batches if counts[b].max() > BATCH_TOPK_MAX))}


def check_plan(stride, counts, f, group_min, sort, row_bytes=0):
    stride, counts, f = np.asarray(stride, np.int64), np.asarray(counts, np.int64), np.asarray(f, dtype=np.uint32)
    batches = plan(stride, counts, f, group_min, sort, row_bytes)
    seen = np.concatenate([b for _k, b in batches]) if batches else np.zeros(0, np.int64)
    assert sorted(seen.tolist()) == list(range(f.size)), "every query exactly once"
    for kind, b in batches:
        assert 0 < b.size <= CHUNK_CAP
        # per-sub-batch bounds: its own largest stride and count
        assert b.size == 1 or b.size * query_bytes(stride[b].max(), counts[b].max(), row_bytes) <= CHUNK_BYTES
        big = counts[b] > BATCH_TOPK_MAX
        assert big.all() or not big.any(), "big and batched counts share a sub-batch"
        # the filter rule of test_search_filters_cpu.plan: by slot, unfiltered first, one slot <=> uniform
        keys = (f[b].astype(np.int64) + 1) & 0xFFFFFFFF
        assert (np.diff(keys) >= 0).all()
        assert (np.unique(keys).size == 1) == (kind == "uniform")
        for k in np.unique(keys):
            run = b[keys == k]
            if sort:  # non-decreasing strides inside a run, the caller's order among equal ones
                assert (np.diff(stride[run]) >= 0).all()
                assert all((np.diff(run[stride[run] == s]) > 0).all() for s in np.unique(stride[run]))
            else:
                assert (np.diff(run) > 0).all()
    return batches


def test_new_symbols_are_exported_and_declared():
    from arroy_amd import _lib
    L = _lib.lib()
    assert L.ah_abi_version() == 7
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert C.sizeof(_lib.AhQueryParams) == 16
    assert C.sizeof(_lib.AhParamsStats) == 48
    assert _lib.tuning_get("AH_SEARCH_PARAMS_SORT")[0] == 1
    import pathlib
    header = (pathlib.Path(__file__).resolve().parent.parent / "include" / "arroy_hip.h").read_text()
    for name in NEW_SYMBOLS + ("ah_query_params", "ah_params_stats"):
        assert name in header, name


def test_refusals_that_need_no_device():
    from arroy_amd import _lib
    L = _lib.lib()
    q = np.zeros((2, 8), np.float32)
    oi, od, oc = np.zeros((2, 9), np.uint32), np.zeros((2, 9), np.float32), np.zeros(2, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    none = C.POINTER(C.c_void_p)()
    two = (C.c_void_p * 2)(None, None)

    def params(*rows):  # (search_k, count, oversampling)
        a = (_lib.AhQueryParams * len(rows))()
        for i, (sk, count, over) in enumerate(rows):
            a[i].search_k, a[i].count, a[i].oversampling = sk, count, over
        return a

    def refused(status, word):
        assert status == 5, status  # AH_ERR_INVALID_ARGUMENT
        assert word in L.ah_last_error().decode(), L.ah_last_error()

    ok = params((0, 3, 0), (100, 9, 2))
    call = L.ah_search_batch_params
    # in the order of the contract: params NULL, a count of 0 or >= 2^31 (the position named), out_stride below the largest count
    refused(call(None, p(q), None, 2, None, 9, none, 0, None, p(oi), p(od), p(oc)), "params is NULL")
    refused(call(None, p(q), None, 2, params((0, 3, 0), (0, 0, 0)), 9, none, 0, None, p(oi), p(od), p(oc)), "params[1].count")
    refused(call(None, p(q), None, 2, params((0, 2**31, 0), (0, 1, 0)), 9, none, 0, None, p(oi), p(od), p(oc)), "params[0].count")
    refused(call(None, p(q), None, 2, ok, 8, none, 0, None, p(oi), p(od), p(oc)), "out_stride")
    # ... each of them before the arguments ah_search_batch_filters looks at
    refused(call(None, None, None, 2, None, 9, none, 0, None, None, None, None), "params is NULL")
    refused(call(None, None, None, 2, ok, 8, none, 0, None, None, None, None), "out_stride")
    # both or neither of queries / query_items, NULL outputs, the filter refusals, a NULL index
    refused(call(None, None, None, 2, ok, 9, none, 0, None, p(oi), p(od), p(oc)), "exactly one")
    refused(call(None, p(q), p(oc), 2, ok, 9, none, 0, None, p(oi), p(od), p(oc)), "exactly one")
    refused(call(None, p(q), None, 2, ok, 9, none, 0, None, None, p(od), p(oc)), "NULL output")
    refused(call(None, p(q), None, 2, ok, 9, none, 2, None, p(oi), p(od), p(oc)), "filters is NULL")
    refused(call(None, p(q), None, 2, ok, 9, two, 2, None, p(oi), p(od), p(oc)), "filter_of_query is NULL")
    for slots, n_filters, word in (([0, NO_FILTER], 0, "names no filter"), ([NO_FILTER, 2], 2, "names no filter"),
                                   ([NO_FILTER, NO_FILTER], 0, "index is NULL")):
        foq = np.array(slots, np.uint32)
        refused(call(None, p(q), None, 2, ok, 9, two, n_filters, p(foq), p(oi), p(od), p(oc)), word)
    refused(call(None, p(q), None, 2, ok, 9, none, 0, None, p(oi), p(od), p(oc)), "index is NULL")
    refused(call(None, p(q), None, 2, ok, 20, none, 0, None, p(oi), p(od), p(oc)), "index is NULL")  # a wider out_stride is fine
    # nq == 0 asks nothing of params; the other arguments are still judged
    refused(call(None, p(q), None, 0, None, 0, none, 0, None, p(oi), p(od), p(oc)), "index is NULL")
    refused(L.ah_index_params_stats(None, C.byref(_lib.AhParamsStats()), 0), "NULL argument")


def test_plan_all_params_equal_is_the_filters_plan():
    rng = np.random.default_rng(5)
    for nq in (1, 5, 700, 2 * CHUNK_CAP + 905):
        for f in (np.full(nq, NO_FILTER), np.zeros(nq), rng.integers(0, 9, nq), rng.integers(0, 3000, nq)):
            for gmin in (1, 16, nq + 1):
                for count in (25, 5000):
                    for sort in (0, 1):
                        got = check_plan(np.full(nq, 1700), np.full(nq, count), f, gmin, sort, row_bytes=800)
                        want = filters_plan(f, gmin)
                        assert [k for k, _ in got] == [k for k, _ in want]
                        assert all(np.array_equal(a, b) for (_k, a), (_j, b) in zip(got, want))
    # ... also where the scratch bound, not the query cap, cuts: 1 Mi-entry buffers, 25 MiB a query, 60 a sub-batch
    per = CHUNK_BYTES // query_bytes(1 << 20, 25, 800)
    assert 1 < per < 100
    got = check_plan(np.full(300, 1 << 20), np.full(300, 25), np.full(300, NO_FILTER), 16, 1, row_bytes=800)
    want = filters_plan(np.full(300, NO_FILTER), 16, chunk=per)
    assert [b.tolist() for _k, b in got] == [b.tolist() for _k, b in want]


def test_plan_one_huge_stride_among_999_small_ones():
    stride = np.full(1000, 1700)
    stride[417] = 1 << 24  # search_k = "everything" on a big forest: 400 MiB of scratch for that query
    counts = np.full(1000, 25)
    f = np.full(1000, NO_FILTER)
    assert 2 * query_bytes(1 << 24, 25, 800) <= CHUNK_BYTES < 5 * query_bytes(1 << 24, 25, 800)
    b = check_plan(stride, counts, f, 16, 1, row_bytes=800)
    assert [x.size for _k, x in b] == [999, 1] and b[1][1].tolist() == [417]
    # unsorted, the big query shrinks the sub-batches around it: the caller's order is kept and cut where the scratch ends
    b0 = check_plan(stride, counts, f, 16, 0, row_bytes=800)
    assert len(b0) > 2 and np.concatenate([x for _k, x in b0]).tolist() == list(range(1000))
    st = stats_of(b, counts, stride)
    assert st == {"calls": 1, "batches": 2, "varied_batches": 0, "queries": 1000, "varied_queries": 0, "big_count_queries": 0}


def test_plan_counts_2048_and_2049_are_split():
    rng = np.random.default_rng(6)
    for gmin in (1, 16, 101):
        for sort in (0, 1):
            counts = np.where(rng.random(100) < 0.4, 2049, 2048)
            stride = rng.choice([300, 1700, 40000], 100)
            b = check_plan(stride, counts, np.full(100, NO_FILTER), gmin, sort, row_bytes=800)
            assert len(b) == 2 and (counts[b[0][1]] == 2048).all() and (counts[b[1][1]] == 2049).all()
            assert stats_of(b, counts, stride)["big_count_queries"] == int((counts == 2049).sum())
    # under filters: the big counts of a slot follow its batched ones, and the left-overs of the two kinds stay apart
    f = rng.integers(0, 4, 100)
    counts = np.where(rng.random(100) < 0.3, 5000, 10)
    stride = rng.choice([300, 1700, 40000], 100)
    for gmin in (1, 8, 16, 101):
        for sort in (0, 1):
            b = check_plan(stride, counts, f, gmin, sort, row_bytes=800)
            st = stats_of(b, counts, stride)
            assert st["big_count_queries"] == int((counts == 5000).sum()) and st["queries"] == 100
    b = check_plan(stride, counts, f, 101, 1, row_bytes=800)
    assert [k for k, _ in b] == ["mixed", "mixed"]


def test_plan_random_calls_keep_the_invariants():
    rng = np.random.default_rng(7)
    for trial in range(40):
        nq = int(rng.integers(1, 900))
        stride = rng.choice([201, 1700, 16300, 32768, 1 << 17, 1 << 20, 1 << 24], nq)
        counts = rng.choice([1, 10, 25, 100, 1024, 1025, 2048, 2049, 5000], nq)
        f = rng.integers(0, int(rng.integers(1, 40)), nq).astype(np.uint32)
        f[rng.random(nq) < 0.2] = NO_FILTER
        for gmin in (1, 16, nq + 1):
            a = check_plan(stride, counts, f, gmin, 1, row_bytes=int(rng.integers(4, 7000)))
            check_plan(stride, counts, f, gmin, 0, row_bytes=800)
            st = stats_of(a, counts, stride)
            assert st["batches"] == len(a) and st["varied_queries"] <= nq
