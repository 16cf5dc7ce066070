"""Updates of a finalized dataset (ah_dataset_update_* / ah_group_update_*): after any chain of updates the dataset behaves bit
for bit like one staged afresh with the resulting items — lengths, headers, vectors, scans, forests and their stats, search and
re-rank — whatever lazily built copies of the rows it held before; bad arguments and failed allocations leave it untouched; and
the Writer mirror reuses its dataset across builds with the same trees and results as staging from scratch every time."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

from arroy_amd import Dataset, DatasetGroup, _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from arroy_amd.index import Database, Reader, Writer  # noqa: E402

OK, INVALID_DIMENSION, DEVICE, OOM, INVALID, MISSING, NOT_FINALIZED, NEED_PREPROCESS = 0, 1, 3, 4, 5, 6, 7, 8
U32_MAX = 0xFFFFFFFF
METRICS = [D.Euclidean, D.Manhattan, D.Cosine, D.DotProduct, D.BinaryQuantizedEuclidean, D.BinaryQuantizedManhattan,
           D.BinaryQuantizedCosine]
SEEDS = [11, 12, 13]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    yield
    _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)


def fresh(dist, dims, items, capacity=None):
    """A dataset staged from scratch with `items` ({id: vector})."""
    ids = np.array(sorted(items), dtype=np.uint32)
    ds = Dataset(dist, dims, len(ids) if capacity is None else capacity)
    if len(ids):
        ds.upload_vectors(ids, np.stack([items[int(i)] for i in ids]))
    if dist.metric == 3:
        ds.preprocess_dot()
    return ds.finalize()


def update(ds, items, remove, upsert, vecs):
    """ds.update_vectors + the same change on the host dict; DotProduct preprocessed again, as Writer::build does."""
    remove = np.array(sorted(set(int(i) for i in remove)), dtype=np.uint32)
    upsert = np.array(sorted(set(int(i) for i in upsert)), dtype=np.uint32)
    vecs = {int(i): v for i, v in zip(upsert, vecs)}
    ds.update_vectors(remove, upsert, np.stack([vecs[int(i)] for i in upsert]) if upsert.size else np.zeros((0, ds.dimensions)))
    for i in remove:
        items.pop(int(i), None)
    items.update(vecs)
    if ds.metric == 3:
        ds.preprocess_dot()


def warm(ds, items):
    """Every lazily built copy of the rows: a build and an index (binary16 / int8), a search, a re-rank and a full scan (packed)."""
    ids = sorted(items)
    if not ids:
        return
    forest = ds.build_forest(SEEDS)
    ix = ds.create_index(forest)
    q = np.stack([items[i] for i in ids[:8]]) + np.float32(0.01)
    ix.search(5, queries=q, search_k=200)
    ds.rerank_batch(q, [ids] * len(q), 5)
    ds.distances(item=ids[0])
    ix.close()
    forest.close()


def strip(stats):
    return {k: v for k, v in stats.items() if not k.startswith("seconds") and k != "host_blob_recycled"}


def assert_same(a, b, items, rng, what=""):
    """Every observable of `a` equals that of `b` (staged afresh with `items`)."""
    ids = np.array(sorted(items), dtype=np.uint32)
    n = len(ids)
    assert len(a) == len(b) == n, what
    assert a.packed_info() == b.packed_info(), what
    if n == 0:
        return
    assert a.read_headers().tobytes() == b.read_headers().tobytes(), what
    for i in rng.choice(ids, min(n, 16), replace=False):
        assert a.item_vector(int(i)).tobytes() == b.item_vector(int(i)).tobytes(), (what, int(i))
    q = int(ids[rng.integers(n)])
    assert a.distances(item=q).tobytes() == b.distances(item=q).tobytes(), what
    assert a.distances(item=q, ids=ids[::3]).tobytes() == b.distances(item=q, ids=ids[::3]).tobytes(), what
    assert a.packed_info() == b.packed_info(), what
    fa, fb = a.build_forest(SEEDS), b.build_forest(SEEDS)
    assert fa.digest()[0] == fb.digest()[0], what
    assert strip(fa.stats) == strip(fb.stats), what
    queries = np.stack([items[int(i)] for i in rng.choice(ids, 12)]) + np.float32(0.01)
    ia, ib = a.create_index(fa), b.create_index(fb)
    ra = ia.search(10, queries=queries, search_k=300, raw=True)
    rb = ib.search(10, queries=queries, search_k=300, raw=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb)), what
    assert ia.stats() == ib.stats(), what
    ia.close(), ib.close(), fa.close(), fb.close()
    lists = [np.sort(rng.choice(ids, min(n, 200), replace=False)) for _ in range(len(queries))]
    a.rerank_stats(reset=True), b.rerank_stats(reset=True)
    ka, kb = a.rerank_batch(queries, lists, 7), b.rerank_batch(queries, lists, 7)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ka, kb)), what
    assert strip(a.rerank_stats()) == strip(b.rerank_stats()), what
    assert a.packed_info() == b.packed_info(), what


def random_change(rng, items, dims, id_space, n_remove, n_new, n_replace, n_both):
    """removals (some absent), new ids below / between / above the present ones, replacements, ids in both lists"""
    present = np.array(sorted(items), dtype=np.int64)
    taken = set(items)
    remove = set(int(i) for i in rng.choice(present, min(n_remove, len(present)), replace=False)) if len(present) else set()
    absent = [int(i) for i in rng.integers(0, id_space, n_remove) if int(i) not in taken]
    remove |= set(absent[: max(1, n_remove // 4)])
    new = set()
    while len(new) < n_new:
        i = int(rng.integers(0, id_space))
        if i not in taken:
            new.add(i)
    replace = set(int(i) for i in rng.choice(present, min(n_replace, len(present)), replace=False)) if len(present) else set()
    both = set(list(remove)[:n_both])
    upsert = sorted(new | replace | both)
    vecs = rng.standard_normal((len(upsert), dims)).astype(np.float32)
    return sorted(remove), upsert, vecs


@pytest.mark.parametrize("dist,dims", [(m, 64) for m in METRICS] + [(D.Cosine, 768), (D.DotProduct, 768)],
                         ids=lambda x: getattr(x, "name", str(x)))
def test_updates_equal_a_fresh_staging(dist, dims):
    rng = np.random.default_rng(dims + dist.metric)
    id_space = 1 << 20
    n = 3000 if dims == 64 else 1500
    ids = rng.choice(id_space, n - 1, replace=False).tolist() + [U32_MAX]  # sparse ids with gaps, and u32::MAX
    items = {int(i): v for i, v in zip(ids, rng.standard_normal((n, dims)).astype(np.float32))}
    a = fresh(dist, dims, items)
    for step in range(3):  # chained: stale state of one update would show in the next
        warm(a, items)
        remove, upsert, vecs = random_change(rng, items, dims, id_space, 150, 120, 90, 20)
        gone = [i for i in remove if i not in set(upsert) and i in items]
        update(a, items, remove, upsert, vecs)
        b = fresh(dist, dims, items)
        assert_same(a, b, items, rng, what=f"{dist.name} step {step}")
        for i in gone[:5]:
            with pytest.raises(_lib.MissingKey):
                a.item_vector(i)
        b.close()
    a.close()


def test_dense_sparse_transitions_and_empty():
    """identity ids (0 .. n-1, no table) -> sparse ids (table) -> dense again -> empty -> items again"""
    rng = np.random.default_rng(3)
    dist, dims, n = D.Cosine, 64, 2000
    items = {i: v for i, v in enumerate(rng.standard_normal((n, dims)).astype(np.float32))}
    a = fresh(dist, dims, items)
    steps = [
        ([], [5_000_000, 5_000_001], rng.standard_normal((2, dims))),  # sparse: no table (too wide), binary search
        ([5_000_000, 5_000_001], [n, n + 1], rng.standard_normal((2, dims))),  # dense again
        ([3, 4, 7], [100_000], rng.standard_normal((1, dims))),  # sparse with a table
        (sorted(set(range(0, 100_001))), [], []),  # empty
        ([], [0, 1, 2], rng.standard_normal((3, dims))),  # an empty finalized dataset updated
        ([], [3, 4, 5, 9], rng.standard_normal((4, dims))),
    ]
    for k, (remove, upsert, vecs) in enumerate(steps):
        warm(a, items)
        update(a, items, remove, upsert, np.asarray(vecs, dtype=np.float32))
        b = fresh(dist, dims, items)
        assert_same(a, b, items, rng, what=f"step {k}")
        b.close()
    a.close()


def test_fast_paths_are_taken_and_equal_a_fresh_staging():
    rng = np.random.default_rng(4)
    for dist in (D.Euclidean, D.BinaryQuantizedCosine, D.DotProduct):
        dims, n = 96, 2500
        ids = np.sort(rng.choice(1 << 16, n, replace=False))
        items = {int(i): v for i, v in zip(ids, rng.standard_normal((n, dims)).astype(np.float32))}
        a = fresh(dist, dims, items, capacity=n + 1000)
        # replace only: the id set does not change (an id removed and upserted again, ids upserted that are present)
        warm(a, items)
        rep = sorted(rng.choice(ids, 300, replace=False).tolist())
        update(a, items, rep[:40], rep, rng.standard_normal((len(rep), dims)).astype(np.float32))
        assert a.update_paths() == {"in_place": 1, "appended": 0, "merged": 0}
        assert_same(a, fresh(dist, dims, items), items, rng, what=f"{dist.name} in place")
        # append only: every new id above the last one, room in the allocation (removals of absent ids change nothing)
        warm(a, items)
        new = list(range(int(ids[-1]) + 1, int(ids[-1]) + 1 + 2 * 400, 2))
        update(a, items, [int(ids[-1]) + 3, 1 << 30], new, rng.standard_normal((len(new), dims)).astype(np.float32))
        assert a.update_paths() == {"in_place": 1, "appended": 1, "merged": 0}
        assert_same(a, fresh(dist, dims, items), items, rng, what=f"{dist.name} append")
        # past the capacity: merged into new arrays
        new = list(range(1 << 20, (1 << 20) + 800))
        update(a, items, [], new, rng.standard_normal((len(new), dims)).astype(np.float32))
        assert a.update_paths() == {"in_place": 1, "appended": 1, "merged": 1}
        assert_same(a, fresh(dist, dims, items), items, rng, what=f"{dist.name} past capacity")
        a.close()


def test_update_records_equals_upload_records():
    rng = np.random.default_rng(5)
    dist, dims, n = D.Cosine, 128, 2000
    hs = dist.header_size()

    def rec(v):
        return b"\0" + np.float32(np.linalg.norm(v)).tobytes()[:hs] + v.tobytes()
    ids = np.sort(rng.choice(50_000, n, replace=False))
    items = {int(i): v for i, v in zip(ids, rng.standard_normal((n, dims)).astype(np.float32))}
    a = Dataset(dist, dims, n)
    a.upload_records(ids, [rec(items[int(i)]) for i in ids])
    a.finalize()
    warm(a, items)
    remove, upsert, vecs = random_change(rng, items, dims, 50_000, 100, 100, 100, 10)
    a.update_records(remove, upsert, [rec(v) for v in vecs])
    for i in remove:
        items.pop(int(i), None)
    items.update({int(i): v for i, v in zip(upsert, vecs)})
    fids = np.array(sorted(items), dtype=np.uint32)
    b = Dataset(dist, dims, len(fids))
    b.upload_records(fids, [rec(items[int(i)]) for i in fids])
    b.finalize()
    assert_same(a, b, items, rng, what="records")
    a.close(), b.close()


def snapshot(ds, ids):
    """What a reader sees (no lazily built copy is made by it: the scan is gathered)."""
    out = [len(ds), ds.read_headers().tobytes() if len(ds) else b""]
    if len(ds):
        q = np.linspace(-1, 1, ds.dimensions, dtype=np.float32)
        out.append(ds.distances(query=q, ids=ids).tobytes())
    return out


def test_refusals_leave_the_dataset_unchanged():
    rng = np.random.default_rng(6)
    dims, n = 64, 1500
    ids = np.sort(rng.choice(10_000, n, replace=False)).astype(np.uint32)
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    items = {int(i): v for i, v in zip(ids, vecs)}
    ds = fresh(D.DotProduct, dims, items)
    before = snapshot(ds, ids)
    one = rng.standard_normal((1, dims)).astype(np.float32)
    L = _lib.lib()

    def status(fn):
        try:
            fn()
        except _lib.ArroyHipError as e:
            return e.status
        return OK
    forest = ds.build_forest(SEEDS)
    ix = ds.create_index(forest)
    assert status(lambda: ds.update_vectors([int(ids[0])], [], [])) == INVALID  # a live index holds row positions
    ix.close()
    assert status(lambda: ds.update_vectors([], [5, 3], rng.standard_normal((2, dims)))) == INVALID  # unsorted
    assert status(lambda: ds.update_vectors([7, 7], [], [])) == INVALID  # duplicate
    assert status(lambda: ds.update_vectors([], [10_001], rng.standard_normal((1, dims + 1)))) == INVALID_DIMENSION
    rec = b"\0" + bytes(8) + one.tobytes()
    assert status(lambda: ds.update_records([], [10_001], [rec + b"\0"])) == INVALID_DIMENSION  # wrong record length
    up = np.array([10_001], dtype=np.uint32)
    assert L.ah_dataset_update_vectors(ds._h, None, 0, up.ctypes.data_as(C.c_void_p), None, 1) == INVALID  # NULL, n > 0
    assert L.ah_dataset_update_vectors(ds._h, None, 3, None, None, 0) == INVALID
    assert snapshot(ds, ids) == before
    unfinalized = Dataset(D.DotProduct, dims, 10)
    unfinalized.upload_vectors([1, 2], rng.standard_normal((2, dims)))
    assert status(lambda: unfinalized.update_vectors([1], [], [])) == NOT_FINALIZED
    unfinalized.close()
    g = DatasetGroup(D.DotProduct, dims, n, [0])
    g.upload_vectors(ids, vecs)
    g.preprocess_dot()
    g.finalize()
    m = g.member(0)
    before_m = snapshot(m, ids)
    assert status(lambda: m.update_vectors([int(ids[0])], [], [])) == INVALID  # a group member: the group call
    assert snapshot(m, ids) == before_m
    g.close()
    # DotProduct: after an update the dataset needs preprocess_dot before a build
    ds.update_vectors([int(ids[0])], [20_000], one)
    assert status(lambda: ds.build_forest(SEEDS)) == NEED_PREPROCESS
    ds.preprocess_dot()
    ds.build_forest(SEEDS).close()
    forest.close()
    ds.close()


def sweep(op, check, limit=2000):
    """op() with the n-th allocation failing, n = 1, 2, ... until a call goes through without the counter firing; every
    status is OK, OUT_OF_MEMORY or DEVICE, and check(status) holds after every call.  Twice: the library's live HBM after the
    second clean call is not above that after the first (what a failing call leaked would still be there)."""
    lives = []
    for _ in range(2):
        for n in range(1, limit):
            _lib.tuning_set("AH_FAIL_ALLOC_AFTER", n)
            try:
                op()
                status = OK
            except _lib.ArroyHipError as e:
                status = e.status
            finally:
                left = _lib.tuning_get("AH_FAIL_ALLOC_AFTER")[0]
                _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
            assert status in (OK, DEVICE, OOM), (n, status)
            check(status)
            if left > 0:
                assert status == OK, n
                break
        else:
            raise AssertionError(f"more than {limit} allocations in one call?")
        lives.append(_lib.device_cache_stats(0)[0])
    assert lives[1] <= lives[0], f"failing updates leaked {lives[1] - lives[0]} bytes of HBM"


class Tracker:
    """The states a dataset may be in during a sweep of one (idempotent) update: before the first successful call it must
    still be its old self after every failure; from then on its updated self."""

    def __init__(self, read, pre):
        self.read, self.pre, self.post = read, pre, None

    def __call__(self, status):
        if status == OK:
            now = self.read(True)
            assert self.post is None or now == self.post
            self.post = now
        elif self.post is None:
            assert self.read(False) == self.pre
        else:
            assert self.read(True) == self.post


def test_updates_survive_every_allocation_failure():
    """The update is idempotent (removing and upserting the same lists again gives the same items), so a sweep can repeat it:
    after every failed call the dataset equals its state before the call, and the clean call succeeds."""
    rng = np.random.default_rng(7)
    dist, dims, n = D.Cosine, 64, 4000
    hs = dist.header_size()
    ids = np.sort(rng.choice(100_000, n, replace=False)).astype(np.uint32)
    items = {int(i): v for i, v in zip(ids, rng.standard_normal((n, dims)).astype(np.float32))}
    remove, upsert, vecs = random_change(rng, items, dims, 100_000, 200, 150, 150, 20)
    recs = [b"\0" + np.float32(np.linalg.norm(v)).tobytes()[:hs] + v.tobytes() for v in vecs]
    final = dict(items)
    for i in remove:
        final.pop(int(i), None)
    final.update({int(i): v for i, v in zip(upsert, vecs)})
    fids = np.array(sorted(final), dtype=np.uint32)
    want = fresh(dist, dims, final)
    for kind in ("vectors", "records"):
        ds = fresh(dist, dims, items)
        warm(ds, items)
        track = Tracker(lambda after, ds=ds: snapshot(ds, fids if after else ids), snapshot(ds, ids))
        if kind == "vectors":
            sweep(lambda: ds.update_vectors(remove, upsert, vecs), track)
            assert track.post == snapshot(want, fids)
        else:
            sweep(lambda: ds.update_records(remove, upsert, recs), track)
            assert len(ds) == len(fids)
        ds.close()
    # a group call (one device listed twice)
    g = DatasetGroup(dist, dims, n, [0, 0])
    g.upload_vectors(ids, np.stack([items[int(i)] for i in ids]))
    g.finalize()
    m0, m1 = g.member(0), g.member(1)

    def read(after):
        got = snapshot(m0, fids if after else ids)
        assert snapshot(m1, fids if after else ids) == got
        return got
    track = Tracker(read, read(False))
    sweep(lambda: g.update_vectors(remove, upsert, vecs), track)
    assert track.post == snapshot(want, fids)
    want.close()
    g.close()


def test_group_update_equals_a_fresh_single_dataset():
    rng = np.random.default_rng(8)
    for dist, dims in ((D.Cosine, 128), (D.BinaryQuantizedEuclidean, 128), (D.DotProduct, 64)):
        n = 3000
        ids = np.sort(rng.choice(1 << 18, n, replace=False)).astype(np.uint32)
        items = {int(i): v for i, v in zip(ids, rng.standard_normal((n, dims)).astype(np.float32))}
        g = DatasetGroup(dist, dims, n, [0, 0])
        g.upload_vectors(ids, np.stack([items[int(i)] for i in ids]))
        if dist.metric == 3:
            g.preprocess_dot()
        g.finalize()
        for step in range(2):
            remove, upsert, vecs = random_change(rng, items, dims, 1 << 18, 200, 150, 100, 20)
            g.update_vectors(remove, upsert, vecs)
            if dist.metric == 3:
                g.preprocess_dot()
            for i in remove:
                items.pop(int(i), None)
            items.update({int(i): v for i, v in zip(upsert, vecs)})
            b = fresh(dist, dims, items)
            want = b.build_forest(SEEDS)
            for i in range(2):
                f = g.member(i).build_forest(SEEDS)
                assert f.digest()[0] == want.digest()[0], (dist.name, step, i)
                f.close()
            _roots, _st, _per, streamed = g.build_stream(SEEDS)
            for t in range(len(SEEDS)):
                assert streamed.canonical(t) == want.canonical(t), (dist.name, step, t)
            want.close()
            b.close()
        g.close()


def _canon(trees, nid):
    nd = trees.nodes[nid]
    if nd[0] == "D":
        return ("D", tuple(int(x) for x in nd[1]))
    return ("S", np.asarray(nd[3]).tobytes(), nd[4], _canon(trees, nd[1]), _canon(trees, nd[2]))


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one device", "group"])
@pytest.mark.parametrize("dist", [D.Cosine, D.DotProduct, D.BinaryQuantizedManhattan], ids=lambda d: d.name)
def test_writer_reuses_its_dataset_and_builds_what_fresh_staging_builds(dist, devices):
    """add / delete / re-add cycles through ArroyBuilder.build: the trees and nns results of a Writer that updates its dataset
    equal those of a Writer that stages from scratch every build (same history, same RNG), and the dataset handle is reused."""
    dims = 32
    rng = np.random.default_rng(9)
    dbs = [Database(dist), Database(dist)]
    writers = [Writer(db, 0, dims) for db in dbs]
    live = set()
    handle = None
    for cycle in range(5):
        ops = []
        for i in rng.choice(3000, 700, replace=False):
            i = int(i)
            if i in live and rng.random() < 0.4:
                ops.append(("del", i, None))
                live.discard(i)
            else:
                ops.append(("add", i, rng.standard_normal(dims).astype(np.float32)))
                live.add(i)
        for w in writers:
            for op, i, v in ops:
                if op == "add":
                    w.add_item(i, v)
                else:
                    w.del_item(i)
        writers[1]._st.dataset = None  # the reference stages from scratch
        for w in writers:
            w.builder(random.Random(cycle), devices=devices).n_trees(3).split_after(40).build()
        st = [w._st for w in writers]
        if cycle == 0:
            handle = st[0].dataset._h.value
        else:
            assert st[0].dataset._h.value == handle, "the dataset is staged afresh instead of updated"
        assert st[0].trees.roots == st[1].trees.roots and sorted(st[0].trees.nodes) == sorted(st[1].trees.nodes), cycle
        for r in st[0].trees.roots:
            assert _canon(st[0].trees, r) == _canon(st[1].trees, r), cycle
        readers = [Reader.open(db, 0) for db in dbs]
        some = sorted(live)[:: max(1, len(live) // 20)]
        for i in some:
            assert readers[0].nns(10).search_k(200).by_item(i) == readers[1].nns(10).search_k(200).by_item(i), (cycle, i)
            v = readers[0].item_vector(i)
            assert v.tobytes() == readers[1].item_vector(i).tobytes()
            assert readers[0].nns(7).by_vector(v + np.float32(0.1)) == readers[1].nns(7).by_vector(v + np.float32(0.1))
    paths = st[0].dataset.update_paths()
    assert sum(paths.values()) == 4, paths
    for w in writers:
        w.clear()


def test_scale_1_5m_x_768_cosine_past_4_gib():
    """1.5M x 768 rows = 4.6 GB (byte offsets past 2^32); 1 % random changes.  The updated dataset's 50-tree forest and the
    search results of 1 000 queries equal those of a fresh staging, and a one-tree forest's search equals the oracle's."""
    from arroy_amd import shard
    rng = np.random.default_rng(10)
    n, dims = 1_500_000, 768
    vecs = O.synth(21, 1, n, dims)
    a = Dataset(D.Cosine, dims, n)
    a.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    a.finalize()
    k = n // 100
    remove = np.sort(rng.choice(n, k // 2, replace=False)).astype(np.uint32)
    replace = np.sort(rng.choice(n, k // 4, replace=False)).astype(np.uint32)
    new = np.arange(n + 7, n + 7 + 2 * (k // 4), 2, dtype=np.uint32)
    upsert = np.union1d(replace, new).astype(np.uint32)
    up_vecs = rng.standard_normal((upsert.size, dims)).astype(np.float32)
    a.update_vectors(remove, upsert, up_vecs)
    keep = np.setdiff1d(np.arange(n, dtype=np.uint32), np.union1d(remove, upsert))
    final_ids = np.union1d(keep, upsert).astype(np.uint32)
    final_vecs = np.empty((final_ids.size, dims), dtype=np.float32)
    pos_keep = np.searchsorted(final_ids, keep)
    final_vecs[pos_keep] = vecs[keep]
    final_vecs[np.searchsorted(final_ids, upsert)] = up_vecs
    del vecs
    b = Dataset(D.Cosine, dims, final_ids.size)
    b.upload_vectors(final_ids, final_vecs)
    b.finalize()
    assert len(a) == len(b) == final_ids.size
    assert a.read_headers().tobytes() == b.read_headers().tobytes()
    seeds = shard.tree_seeds(5, range(50))
    fa, fb = a.build_forest(seeds), b.build_forest(seeds)
    assert fa.digest()[0] == fb.digest()[0]
    queries = final_vecs[rng.choice(final_ids.size, 1000, replace=False)] + np.float32(0.02)
    ia, ib = a.create_index(fa), b.create_index(fb)
    ra, rb = ia.search(10, queries=queries, search_k=1000, raw=True), ib.search(10, queries=queries, search_k=1000, raw=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
    ia.close(), ib.close(), fa.close(), fb.close()
    b.close()
    # the oracle on one tree of the updated dataset
    one = a.build_forest(seeds[:1])
    ix = a.create_index(one)
    got = ix.search(10, queries=queries[:6], search_k=2000, raw=True)
    oracle = O.Data(O.COSINE, final_vecs, ids=final_ids)
    for qi in range(6):
        qv, qh = oracle.query_leaf(queries[qi])
        want, _ = O.search(oracle, one, qv, qh, 10, 2000, want_candidates=False)
        assert list(got[0][qi, :got[2][qi]]) == [i for i, _ in want], qi
        assert got[1][qi, :got[2][qi]].tobytes() == np.array([d for _, d in want], dtype=np.float32).tobytes(), qi
    ix.close(), one.close(), a.close()
