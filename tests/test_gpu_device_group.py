"""Device groups (include/arroy_hip.h, "Device groups"): one replica of the dataset per listed device, staged from one host
pass, and one forest built over all of them (tree t on member t mod G).  On a one-GPU box the groups list device 0 several
times ([0, 0], [0, 0, 0]): every member is then a replica of its own on that GPU, built by a host thread of its own, which
exercises the whole fan-out and the renumbering of the stream; a [0, 1] variant runs where two devices exist.

Every member must hold exactly what a dataset staged alone holds, and a group build must stream exactly the forest
ah_build_forest_stream builds on one dataset with the same seeds, under the same sink contract."""
import ctypes as C
import threading

import numpy as np
import pytest

import test_gpu_parity as P
from oracle import oracle as O
from test_gpu_parity import make_data

pytestmark = pytest.mark.gpu

from arroy_amd import _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

CANCELLED, OK, DEVICE, OOM = 2, 0, 3, 4


@pytest.fixture(scope="module", autouse=True)
def _imports():
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    P.D, P.O = D, O


def _group(cls, dims, n, devices, vecs=None, ids=None, records=None, preprocessed=None):
    from arroy_amd import DatasetGroup
    g = DatasetGroup(cls, dims, n, devices)
    half = n // 2
    if records is None:
        g.upload_vectors(ids[:half], vecs[:half])  # two calls: chunked append
        g.upload_vectors(ids[half:], vecs[half:])
    else:
        g.upload_records(ids[:half], records[:half], preprocessed=preprocessed)
        g.upload_records(ids[half:], records[half:], preprocessed=preprocessed)
    return g


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_dataset(single, member, ids, rng):
    n = len(single)
    assert len(member) == n
    assert single.read_headers().tobytes() == member.read_headers().tobytes()
    for item in rng.choice(ids, size=min(24, n), replace=False):
        assert _bits(single.item_vector(int(item))).tolist() == _bits(member.item_vector(int(item))).tolist()
    for q in rng.choice(ids, size=3, replace=False):
        assert _bits(single.distances(item=int(q))).tolist() == _bits(member.distances(item=int(q))).tolist()


def _shapes():
    return [(cls, 40 if cls.metric < 4 else 130) for cls in D.ALL]


@pytest.mark.parametrize("cls,dims", _shapes(), ids=[c.name for c, _ in _shapes()])
def test_every_member_holds_what_a_dataset_staged_alone_holds(cls, dims):
    """Staging through upload_vectors and upload_records (gathered once, sent to every member) on all seven metrics."""
    from arroy_amd import Dataset
    n = 2500
    rng = np.random.default_rng(dims + cls.metric)
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    ids = (np.arange(n, dtype=np.uint32) * 3 + 1)  # not 0..n-1: the id table path
    single = Dataset(cls, dims, n)
    single.upload_vectors(ids, vecs)
    if cls.metric == 3:
        single.preprocess_dot()
    single.finalize()
    oracle = O.Data(cls.metric, vecs)
    records = [b"\0" + oracle.headers[i].tobytes() + oracle.codec[i].tobytes() for i in range(n)]
    for devices, kw in (([0, 0], dict(vecs=vecs)), ([0, 0, 0], dict(records=records, preprocessed=False))):
        g = _group(cls, dims, n, devices, ids=ids, **kw)
        if cls.metric == 3:
            g.preprocess_dot()
        g.finalize()
        for i in range(len(devices)):
            _same_dataset(single, g.member(i), ids, rng)
        g.close()
    single.close()


def _reference(cls, dims, n, seed, seeds, split_after=0):
    ds, oracle, vecs, ids = make_data(cls, n, dims, seed=seed)
    _roots, stats, want = ds.build_forest_stream(seeds, split_after=split_after)
    return ds, oracle, vecs, ids, [want.canonical(t) for t in range(len(seeds))], stats


def _checked_sink(got, entered):
    """StreamedForest.take behind a NON-blocking lock: a second thread inside the sink fails the test."""
    lock = threading.Lock()

    def sink(b):
        if not lock.acquire(blocking=False):
            entered.append("concurrent")
            return 1
        try:
            return got.take(b)
        finally:
            lock.release()
    return sink


def _assert_stream_contract(got, roots, n_trees):
    n_nodes = len(got.splits) + len(got.leaves)
    assert sorted(list(got.splits) + list(got.leaves)) == list(range(n_nodes))  # dense, unique (take() asserts "once")
    for i, (_nb, left, right, tree, depth, _count) in got.splits.items():
        assert right == left + 1 and left > i  # children consecutive, numbered (hence delivered) after the parent
        for c in (left, right):
            child = got.splits.get(c)
            assert ((child[3], child[4]) if child else got.leaves[c][1:]) == (tree, depth + 1)
    # tree indices are global, the roots in tree order
    trees_seen = {v[3] for v in got.splits.values()} | {v[1] for v in got.leaves.values()}
    assert trees_seen == set(range(n_trees))
    for t in range(n_trees):
        r = int(roots[t])
        assert (got.splits[r][3] if r in got.splits else got.leaves[r][1]) == t
        assert (got.splits[r][4] if r in got.splits else got.leaves[r][2]) == 0


@pytest.mark.parametrize("cls,dims,n", [(D.Cosine, 64, 9000), (D.Euclidean, 48, 7000), (D.DotProduct, 40, 6000),
                                        (D.BinaryQuantizedManhattan, 128, 6000)],
                         ids=["cosine", "euclidean", "dot", "bq_manhattan"])
def test_group_forest_equals_the_single_device_forest(cls, dims, n):
    from arroy_amd import DatasetGroup
    seeds = list(range(500, 510))
    ds, oracle, vecs, ids, want, _ = _reference(cls, dims, n, dims + n, seeds)
    # the oracle builds the same trees (as test_gpu_stream.py checks for the single-device stream)
    assert want[0] == oracle.build_tree(0, seeds[0]).canonical()
    assert want[9] == oracle.build_tree(0, seeds[9]).canonical()
    groups = [[0, 0], [0, 0, 0]]
    import arroy_amd
    if arroy_amd.device_count() >= 2:
        groups.append([0, 1])
    for devices in groups:
        G = len(devices)
        g = DatasetGroup(cls, dims, n, devices)
        g.upload_vectors(ids, vecs)
        if cls.metric == 3:
            g.preprocess_dot()
            for i in range(G):
                assert g.member(i).read_headers().tobytes() == ds.read_headers().tobytes()
        g.finalize()
        for n_trees in sorted({1, G - 1, G, 10}):
            from arroy_amd.dataset import StreamedForest
            got = StreamedForest(cls, dims)
            entered = []
            roots, stats, per, _ = g.build_stream(seeds[:n_trees], sink=_checked_sink(got, entered))
            got.roots = roots
            assert not entered, "the sink was entered by two threads at once"
            assert [got.canonical(t) for t in range(n_trees)] == want[:n_trees], (devices, n_trees)
            _assert_stream_contract(got, roots, n_trees)
            assert len(per) == G and stats["split_nodes"] == sum(p["split_nodes"] for p in per) == len(got.splits)
            assert stats["descendant_nodes"] == len(got.leaves)
        g.close()
    ds.close()


def test_group_of_small_datasets_is_one_leaf_per_tree():
    from arroy_amd import DatasetGroup
    ds, _oracle, vecs, ids = make_data(D.Euclidean, 500, 32, seed=3)
    g = DatasetGroup(D.Euclidean, 32, 500, [0, 0])
    g.upload_vectors(ids, vecs)
    g.finalize()
    roots, _stats, _per, got = g.build_stream([4, 5, 6], split_after=600)
    assert sorted(roots.tolist()) == [0, 1, 2] and not got.splits
    assert [got.leaves[int(r)][0] for r in roots] == [tuple(int(x) for x in ids)] * 3
    assert [got.leaves[int(roots[t])][1] for t in range(3)] == [0, 1, 2]
    g.close()
    ds.close()


def test_stopping_a_group_build_and_building_again():
    from arroy_amd import BuildCancelled, DatasetGroup
    seeds = list(range(40, 46))
    ds, _oracle, vecs, ids, want, _ = _reference(D.Cosine, 48, 8000, 77, seeds, split_after=30)
    g = DatasetGroup(D.Cosine, 48, 8000, [0, 0, 0])
    g.upload_vectors(ids, vecs)
    g.finalize()
    late = []

    def watched(fn):
        """fn as a sink that records any call made after the build returned (the event is set once it has)"""
        returned = threading.Event()

        def sink(b):
            if returned.is_set():
                late.append(1)
                return 1
            return fn(b)
        return sink, returned
    calls = []

    def stop_at_fifth(b):
        calls.append(1)
        return 9 if len(calls) == 5 else 0
    sink, returned = watched(stop_at_fifth)
    with pytest.raises(BuildCancelled) as e:
        g.build_stream(seeds, sink=sink, split_after=30)
    returned.set()
    assert "sink" in e.value.message and len(calls) == 5
    # a cancel flag raised from the progress callback (called on the calling thread)
    flag = C.c_int(0)
    levels = []

    def progress(level, nodes_done, items_routed):
        levels.append(threading.get_ident())
        flag.value = 1
    sink, returned = watched(lambda b: 0)
    with pytest.raises(BuildCancelled):
        g.build_stream(seeds, sink=sink, split_after=30, cancel=flag, progress=progress)
    returned.set()
    assert levels and set(levels) == {threading.get_ident()}
    # an exception inside the sink comes back to the caller
    sink, returned = watched(lambda b: 1 // 0)
    with pytest.raises(ZeroDivisionError):
        g.build_stream(seeds, sink=sink, split_after=30)
    returned.set()
    import time
    time.sleep(0.05)
    assert not late, "a sink call after the build returned"
    # progress never decreases, and the group still builds the right forest
    seen = []
    roots, _stats, _per, got = g.build_stream(seeds, split_after=30, progress=lambda *a: seen.append(a[1:]))
    assert [got.canonical(t) for t in range(len(seeds))] == want
    assert seen and all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(seen, seen[1:]))
    g.close()
    ds.close()


def test_allocation_faults_of_the_group_entry_points():
    """AH_FAIL_ALLOC_AFTER = 1, 2, ... over creation, staging, reservation, finalize and the build of a group (the mechanism of
    test_gpu_faults.py): a status code every time, never a crash — and the SAME group that met the fault, its failed call
    simply made again, ends up building the right forest."""
    from arroy_amd import DatasetGroup
    seeds = [7, 8, 9]
    ds, _oracle, vecs, ids, want, _ = _reference(D.Euclidean, 32, 3000, 12, seeds)
    half = 1500
    failed_steps = set()

    def step(name, fn):
        try:
            return fn()
        except _lib.ArroyHipError as e:
            assert e.status in (DEVICE, OOM, CANCELLED), (name, e.status, e.message)
            assert e.message, name
            failed_steps.add(name)
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)  # (it has fired; nothing else fails) — the same call again
        return fn()

    for n in range(1, 3000):
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", n)
        try:
            g = step("create", lambda: DatasetGroup(D.Euclidean, 32, 3000, [0, 0]))
            step("upload 1", lambda: g.upload_vectors(ids[:half], vecs[:half]))
            step("reserve", lambda: g.reserve_build(len(seeds)))
            step("upload 2", lambda: g.upload_vectors(ids[half:], vecs[half:]))
            step("finalize", g.finalize)
            got = step("build", lambda: g.build_stream(seeds)[3])
            left = _lib.tuning_get("AH_FAIL_ALLOC_AFTER")[0]
        finally:
            _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        assert [got.canonical(t) for t in range(len(seeds))] == want, (n, sorted(failed_steps))
        # the group that met the fault builds the right forest again, too
        _r, _s, _p, again = g.build_stream(seeds)
        assert [again.canonical(t) for t in range(len(seeds))] == want, n
        g.close()
        if left > 0:  # the counter never fired: every allocation of the sequence has failed once
            break
    else:
        raise AssertionError("more than 3000 allocations?")
    assert {"create", "upload 1", "upload 2", "build"} <= failed_steps, failed_steps  # (finalize of 0..n-1 ids allocates nothing)
    ds.close()


def test_member_handles_refuse_calls_that_change_one_replica():
    import ctypes

    from arroy_amd import DatasetGroup
    ds, _oracle, vecs, ids = make_data(D.DotProduct, 400, 32, seed=8)
    g = DatasetGroup(D.DotProduct, 32, 400, [0, 0])
    g.upload_vectors(ids[:200], vecs[:200])
    L = _lib.lib()
    h = g.member(1)._h
    INVALID = 5
    one = np.array([300], dtype=np.uint32)
    assert L.ah_dataset_upload_vectors(h, one.ctypes.data_as(ctypes.c_void_p), vecs[300:301].ctypes.data_as(ctypes.c_void_p), 1) == INVALID
    assert L.ah_dataset_fill_synthetic(h, 1, 1, 10) == INVALID
    assert L.ah_dataset_set_preprocessed(h, 1) == INVALID
    assert L.ah_preprocess_dot(h, None) == INVALID
    assert L.ah_dataset_finalize(h) == INVALID
    assert L.ah_dataset_destroy(h) == INVALID
    assert b"device group" in L.ah_last_error()
    # the group itself goes on as if nothing happened
    g.upload_vectors(ids[200:], vecs[200:])
    g.preprocess_dot()
    g.finalize()
    for i in range(2):
        assert g.member(i).read_headers().tobytes() == ds.read_headers().tobytes()
    g.close()
    ds.close()


@pytest.mark.parametrize("cls", [D.Cosine, D.DotProduct], ids=["cosine", "dot"])
def test_search_on_a_member_equals_a_one_device_index(cls):
    from arroy_amd import DatasetGroup
    from arroy_amd.index import TreeStore
    dims, n = 48, 6000
    seeds = list(range(60, 66))
    ds, _oracle, vecs, ids = make_data(cls, n, dims, seed=31)
    forest = ds.build_forest(seeds)
    one = ds.create_index(forest)
    g = DatasetGroup(cls, dims, n, [0, 0])
    g.upload_vectors(ids, vecs)
    if cls.metric == 3:
        g.preprocess_dot()
        h0 = g.member(0).read_headers()
        assert h0.tobytes() == g.member(1).read_headers().tobytes() == ds.read_headers().tobytes()
    g.finalize()
    _roots, _stats, _per, got = g.build_stream(seeds)
    trees = TreeStore()
    for t in range(len(seeds)):
        root = trees.next_id()
        trees.import_streamed_tree(got, t, root_id=root)
        trees.roots.append(root)
    single = TreeStore()
    for t in range(len(seeds)):
        root = single.next_id()
        single.import_tree(forest, t, root_id=root)
        single.roots.append(root)
    from arroy_amd import Index
    view, keep = trees.to_view(cls, dims)
    idx = Index(g.member(1), None, view=view)
    sview, skeep = single.to_view(cls, dims)
    sidx = Index(ds, None, view=sview)
    queries = vecs[[1, 17, 999, 4321]] + np.float32(1e-3)
    a = idx.search(10, queries=queries, search_k=400)
    b = sidx.search(10, queries=queries, search_k=400)
    c = one.search(10, queries=queries, search_k=400)
    assert [[(i, float(np.float32(d)).hex()) for i, d in r] for r in a] == [[(i, float(np.float32(d)).hex()) for i, d in r] for r in b]
    assert [[i for i, _ in r] for r in a] == [[i for i, _ in r] for r in c]
    idx.close()
    sidx.close()
    one.close()
    del keep, skeep
    forest.close()
    g.close()
    ds.close()


def test_arroy_builder_on_devices_builds_the_same_index():
    import random

    from arroy_amd.index import Database, Reader, Writer
    rng = np.random.default_rng(5)
    vecs = rng.standard_normal((3000, 32)).astype(np.float32)
    results = []
    for devices in (None, [0, 0]):
        db = Database(D.Euclidean)
        w = Writer(db, 0, 32)
        for i, v in enumerate(vecs):
            w.add_item(i, v)
        w.builder(random.Random(42), devices=devices).n_trees(5).build()
        r = Reader.open(db, 0)
        results.append([r.nns(10).by_item(i) for i in (0, 7, 2999)])
    assert results[0] == results[1]


def test_concurrent_replication_of_an_unfinalized_source():
    """ah_dataset_replicate flushes the source under its staging lock: several threads may replicate it at once."""
    n, dims = 4000, 64
    rng = np.random.default_rng(9)
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    for _round in range(3):
        _replicate_concurrently(vecs, n, dims)


def _replicate_concurrently(vecs, n, dims):
    from arroy_amd import Dataset
    src = Dataset(D.Cosine, dims, n)
    src.upload_vectors(np.arange(n, dtype=np.uint32), vecs)  # still in flight: not finalized, not flushed
    out, errors = [None] * 6, []

    def rep(i):
        try:
            out[i] = src.replicate(0)
        except Exception as e:  # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=rep, args=(i,)) for i in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    src.finalize()
    want = src.read_headers().tobytes()
    for r in out:
        r.finalize()
        assert r.read_headers().tobytes() == want
        assert _bits(r.distances(item=11)).tolist() == _bits(src.distances(item=11)).tolist()
        r.close()
    src.close()
