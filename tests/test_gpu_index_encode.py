"""ah_index_encode_nodes (arroy_amd/csrc/index_encode.hip): the nodes of a resident index as the `NodeCodec` values LMDB stores.
Every comparison is byte equality with arroy_amd/node_codec.py — values_of_export over Index.export(), or the values an index
was opened from; there are no tolerances."""
import random

import numpy as np
import pytest

import node_codec_cases as cases
from test_gpu_faults import DEVICE, OOM, sweep

pytestmark = pytest.mark.gpu

from arroy_amd import Dataset, Index, _lib, node_codec  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from arroy_amd import index as I  # noqa: E402

INVALID_ARGUMENT = 5
BASE = 0x01020304


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"


def make(cls, n, dims, seed, ids=None, duplicates=0):
    vecs = np.random.default_rng(seed).standard_normal((n, dims)).astype(np.float32)
    if duplicates:
        vecs[100:100 + duplicates] = vecs[100]  # identical rows: nodes over them have `normal: None`
    ds = Dataset(cls, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32), vecs)
    if cls.metric == 3:
        ds.preprocess_dot()
    ds.finalize()
    return ds, vecs


def spread(nid: int) -> int:
    """Every other node id shifted further: strictly increasing, and no id is its own rank."""
    return BASE + nid + 3 * (nid // 2)


def stream_values(ds, seeds, split_after):
    """(node ids, values, root ids) of a streamed build, the values made by node_codec.py, the node ids spread."""
    roots, _stats, got = ds.build_forest_stream(seeds, split_after=split_after)
    nids = sorted(list(got.splits) + list(got.leaves))
    values = []
    for nid in nids:
        if nid in got.splits:
            nb, left, right = got.splits[nid][:3]
            values.append(node_codec.encode_split(spread(left), spread(right), nb))
        else:
            values.append(node_codec.encode_descendants(np.array(got.leaves[nid][0], dtype=np.uint32)))
    return [spread(n) for n in nids], values, [spread(int(r)) for r in roots]


def reference(ix, node_ids=None):
    ds = ix.dataset
    return node_codec.values_of_export(ix.export(), ds.distance, ds.dimensions, node_ids)


def assert_whole_index(ix, node_ids=None):
    """encode_nodes(None) == values_of_export(export), the stats counting what the export holds; returns the values."""
    want = reference(ix, node_ids)
    got, st = ix.encode_nodes(None, node_ids=node_ids, want_stats=True)
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (len(bad), bad[:5], got[bad[0]][:40].hex(), want[bad[0]][:40].hex())
    kinds = ix.export(normals=False)["nodes"]["kind"]
    assert (st["n_values"], st["n_split"], st["n_descendants"], st["n_free"]) == (
        len(want), int((kinds == 2).sum()), int((kinds == 1).sum()), int((kinds == 0).sum()))
    assert st["value_bytes"] == sum(len(v) for v in want) and st["pieces"] >= 1
    return got


# ---- 1. round trip ---------------------------------------------------------------------------------------------------------
ROUND_TRIP = [(D.Euclidean, 32), (D.Cosine, 256), (D.DotProduct, 32), (D.Manhattan, 30), (D.BinaryQuantizedEuclidean, 64)]


@pytest.mark.parametrize("cls,dims", ROUND_TRIP, ids=[f"{m.__name__}-{d}" for m, d in ROUND_TRIP])
def test_round_trip_of_a_streamed_build(cls, dims):
    """20 000 rows in leaves of at most 8 ids: thousands of nodes, so several 1024-length tiles of the scan.  Manhattan-30: a
    120-byte vector in a 128-byte row; BinaryQuantizedEuclidean-64: one 64-bit word a row.  A 1 MiB piece (AH_READBACK_MB at
    its floor of 2) cuts the 1037-byte values of Cosine-256 into several pieces."""
    ds, _vecs = make(cls, 20000, dims, seed=dims + cls.metric)
    node_ids, values, roots = stream_values(ds, [77], split_after=8)
    assert len(values) > 3 * 1024
    ix = Index.from_encoded(ds, node_ids, values, roots)
    with _lib.tuning(AH_READBACK_MB=1):
        got, st = ix.encode_nodes(None, node_ids=node_ids, want_stats=True)
    assert got == values
    assert st["n_values"] == len(values) and st["n_free"] == 0 and st["value_bytes"] == sum(len(v) for v in values)
    assert st["n_split"] == sum(v[0] == 2 for v in values) and st["n_descendants"] == sum(v[0] == 1 for v in values)
    if cls is D.Cosine:
        assert st["value_bytes"] > 2 << 20 and st["pieces"] > 1, st
    assert got == reference(ix, node_ids)
    ix.close()
    ds.close()


# ---- 2. every maintenance state ----------------------------------------------------------------------------------------------
def put_values(delta, before, dist, dims):
    """The values of a delta's put nodes (node ids = node slots): a Descendants node from the delta's ids, a split node from the
    delta's children and the normal its value had before the step."""
    out = []
    for slot, nd in zip(delta["put_index"], delta["put"]):
        if int(nd["kind"]) == 1:
            off, cnt = int(nd["offset"]), int(nd["count"])
            out.append(node_codec.encode_descendants(delta["desc"][off:off + cnt]))
        else:
            old = node_codec.decode_value(dist, dims, before[int(slot)])
            assert old[0] == "S"
            out.append(node_codec.encode_split(int(nd["left"]), int(nd["right"]), old[3]))
    return out


@pytest.mark.parametrize("cls,dims", [(D.Euclidean, 16), (D.BinaryQuantizedEuclidean, 70)], ids=["Euclidean-16", "BQEuclidean-70"])
def test_every_maintenance_state(cls, dims):
    n, seeds, split_after = 3000, [5, 6, 7], 8
    ds, _vecs = make(cls, n, dims, seed=3)
    forest = ds.build_forest(seeds, split_after=split_after)
    ix = Index(ds, forest)
    forest.close()
    before = assert_whole_index(ix)
    # delete: free slots, shrunken lists, split nodes with new children
    gone = np.arange(0, n, 3, dtype=np.uint32)
    delta = ix.delete_items(gone, split_after)
    assert delta["removed"].size and delta["put_index"].size and (delta["put"]["kind"] == 2).any()
    assert ix.encode_nodes(delta["put_index"]) == put_values(delta, before, cls, dims)
    before = assert_whole_index(ix)
    assert sum(v == b"" for v in before) == delta["removed"].size
    # insert: the lists grow
    delta = ix.insert_items(gone, seeds)
    assert delta["put_index"].size
    assert ix.encode_nodes(delta["put_index"]) == put_values(delta, before, cls, dims)
    assert_whole_index(ix)
    # graft: the sub-tree of the largest list takes its place, the index is renumbered
    ex = ix.export(normals=False)
    leaves = np.flatnonzero(ex["nodes"]["kind"] == 1)
    target = int(leaves[np.argmax(ex["nodes"]["count"][leaves])])
    lo, cnt = int(ex["nodes"]["offset"][target]), int(ex["nodes"]["count"][target])
    assert cnt > 4
    sub = ds.build_subtrees([ex["descendants"][lo:lo + cnt]], [99], split_after=2)
    n_before = ix.export_info()["n_nodes"]
    ix.graft(sub.view_struct(), [target])
    sub.close()
    assert ix.export_info()["n_nodes"] != n_before
    assert_whole_index(ix)
    # drop_trees: a whole tree of free slots
    delta = ix.drop_trees(1)
    values = assert_whole_index(ix)
    assert sum(v == b"" for v in values) >= delta["removed"].size > 0
    # compact: no free slot, the normal rows renumbered
    stats = ix.compact()
    assert stats["moved"]
    values = assert_whole_index(ix)
    assert all(values)
    ix.close()
    ds.close()


# ---- 3. containers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 37])
def test_lists_with_bitmap_containers_and_with_several_containers(stride):
    """Leaves of up to 6000 ids: with ids 0 .. 19 999 one of more than 4096 lies in one container, a bitmap; with ids 37 i the
    lists spread over a dozen containers."""
    n = 20000
    ds, _vecs = make(D.Euclidean, n, 8, seed=stride, ids=np.arange(n, dtype=np.uint32) * stride)
    forest = ds.build_forest([1, 2, 3], split_after=6000)
    ix = Index(ds, forest)
    forest.close()
    values = assert_whole_index(ix)
    lists = [node_codec.decode_value(D.Euclidean, 8, v)[1] for v in values if v[0] == 1]
    cards = [np.unique(l >> 16, return_counts=True)[1] for l in lists]
    if stride == 1:
        assert any((c > 4096).any() for c in cards)
    else:
        assert max(len(c) for c in cards) >= 4
    ix.close()
    ds.close()


def test_one_node_trees_and_an_emptied_root():
    ids = cases.edge_lists()["bitmap_array_one"]  # a bitmap, an array of 4096 and a container of one id
    ds, _vecs = make(D.Euclidean, ids.size, 8, seed=8, ids=ids)
    value = node_codec.encode_descendants(ids)
    ix = Index.from_encoded(ds, [5], [value], [5])
    assert ix.encode_nodes(None, node_ids=[5]) == [value] and ix.encode_nodes([0, 0]) == [value, value]
    assert_whole_index(ix)
    ix.close()
    ds.close()
    ds, _vecs = make(D.Euclidean, 20, 8, seed=9)
    ix = Index.from_encoded(ds, [7], [node_codec.encode_descendants(np.arange(20))], [7])
    ix.delete_items(np.arange(20, dtype=np.uint32), 8)
    values = assert_whole_index(ix)
    root = int(ix.export(normals=False)["roots"][0])
    assert values[root] == node_codec.encode_descendants([]) and len(values[root]) == 9
    ix.close()
    ds.close()


def test_identical_rows_give_split_values_without_a_normal():
    ds, _vecs = make(D.Cosine, 900, 24, seed=4, duplicates=40)
    forest = ds.build_forest([11, 12], split_after=8)
    ix = Index(ds, forest)
    forest.close()
    values = assert_whole_index(ix)
    assert any(len(v) == 9 and v[0] == 2 for v in values) and any(len(v) > 9 and v[0] == 2 for v in values)
    ix.close()
    ds.close()


# ---- 4. id tables and order, 5. refusals, 6. allocation failures: one index ---------------------------------------------------
@pytest.fixture(scope="module")
def world():
    n, dims, seeds = 3000, 16, [21, 22, 23]
    ds, vecs = make(D.DotProduct, n, dims, seed=6)
    forest = ds.build_forest(seeds, split_after=8)
    ix = Index(ds, forest)
    forest.close()
    ident = reference(ix)
    queries = vecs[np.arange(16) * 131 % n] + np.float32(1e-3)
    yield ds, ix, ident, queries
    ix.close()
    ds.close()


def test_id_tables_and_order(world):
    ds, ix, ident, _q = world
    nn = len(ident)
    rng = np.random.default_rng(2)
    table = (rng.permutation(nn).astype(np.uint32) * np.uint32(3) + np.uint32(17))
    nodes = ix.export(normals=False)["nodes"]
    table[int(nodes["left"][np.flatnonzero(nodes["kind"] == 2)[0]])] = 0xFFFFFFFE
    want = reference(ix, table)
    assert any(v[0] == 2 and v[1:5] == b"\xff\xff\xff\xfe" for v in want)
    assert ix.encode_nodes(None, node_ids=table) == want
    based = reference(ix, np.arange(nn, dtype=np.uint64) + BASE)
    assert based != ident and ix.encode_nodes(None, base=BASE) == based
    # the largest base that still fits
    top = 0xFFFFFFFF - (nn - 1)
    assert ix.encode_nodes(None, base=top) == reference(ix, np.arange(nn, dtype=np.uint64) + top)
    # any order, repeats
    order = np.concatenate([np.arange(nn)[::-1], [3, 3, 0, nn - 1, 3], rng.integers(0, nn, 50)]).astype(np.uint32)
    assert ix.encode_nodes(order) == [ident[i] for i in order]
    assert ix.encode_nodes(order, node_ids=table) == [want[i] for i in order]
    assert ix.encode_nodes(order[:7], base=BASE) == [based[i] for i in order[:7]]
    # the sizes alone
    ends = ix.encode_nodes(order, sizes_only=True)
    assert ends.dtype == np.uint64 and ends.tolist() == np.concatenate([[0], np.cumsum([len(ident[i]) for i in order])]).tolist()
    ends, st = ix.encode_nodes(None, sizes_only=True, want_stats=True)
    assert ends.tolist() == np.concatenate([[0], np.cumsum([len(v) for v in ident])]).tolist() and st["pieces"] == 0
    # the call reads only: legal with a live filter, which serves as before afterwards
    keep = ix.make_filter(np.arange(0, 3000, 3, dtype=np.uint32), sorted=True)
    served = ix.search(5, queries=_q, search_k=300, candidates=keep, raw=True)
    assert ix.encode_nodes(None) == ident
    again = ix.search(5, queries=_q, search_k=300, candidates=keep, raw=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, served))
    keep.close()
    # nothing listed
    got, st = ix.encode_nodes(np.zeros(0, np.uint32), want_stats=True)
    assert got == [] and st["n_values"] == 0 and st["value_bytes"] == 0
    assert ix.encode_nodes([], sizes_only=True).tolist() == [0]


def raw_call(ix, indices, n, id_of=None, base=0, out=None, cap=0):
    """The C call itself: (status, message, offsets)."""
    L = _lib.lib()
    idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32)
    ends = np.full(n + 1, 0xA5A5A5A5, dtype=np.uint64)
    status = L.ah_index_encode_nodes(ix._h, None if idx is None else idx.ctypes.data, n if idx is None else idx.size,
                                     None if id_of is None else id_of.ctypes.data, base, None if out is None else out.ctypes.data, cap,
                                     ends.ctypes.data, None)
    return status, L.ah_last_error().decode(), ends


def test_refusals_write_nothing_and_leave_the_index_serving(world):
    ds, ix, ident, queries = world
    nn = len(ident)
    need = sum(len(v) for v in ident)
    served = ix.search(10, queries=queries, search_k=400, raw=True)

    def still_serves():
        again = ix.search(10, queries=queries, search_k=400, raw=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, served))

    def refused(msg, indices, n, **kw):
        out = np.full(need + 64, 0xA5, dtype=np.uint8)
        status, err, _ends = raw_call(ix, indices, n, out=out, cap=need, **kw)
        assert status == INVALID_ARGUMENT and msg in err, (status, err)
        assert bool(np.all(out == 0xA5)), "a refused call wrote into out_values"
        still_serves()

    # an index past the node slots: the first offender by position is named
    refused(f"node_indices[2] = {nn}", [0, 1, nn, 5, nn + 7], 5)
    refused("node_indices[0] = 4294967295", [0xFFFFFFFF], 1)
    # an id beyond 32 bits: the listed node's own, and a child's alone
    refused("passes 2^32 - 1", None, nn, base=0xFFFFFFFF - (nn - 2))
    nodes = ix.export(normals=False)["nodes"]
    splits = np.flatnonzero(nodes["kind"] == 2)
    below = splits[np.maximum(nodes["left"][splits], nodes["right"][splits]) > splits]  # a child's id alone passes, where one is
    split = int(below[0] if below.size else splits[0])
    top = int(max(split, nodes["left"][split], nodes["right"][split]))
    refused("passes 2^32 - 1", [split], 1, base=0xFFFFFFFF - top + 1)
    status, _err, _ends = raw_call(ix, [split], 1, base=0xFFFFFFFF - top)
    assert status == 0
    # out_cap one byte short, and exactly enough (the wrapper checks that nothing lands past the values)
    out = np.full(need + 64, 0xA5, dtype=np.uint8)
    status, err, ends = raw_call(ix, None, nn, out=out, cap=need - 1)
    assert status == INVALID_ARGUMENT and f"need {need} bytes, out_cap is {need - 1}" in err and bool(np.all(out == 0xA5))
    assert int(ends[nn]) == need  # (the offsets are the answer to "how much?")
    with pytest.raises(_lib.ArroyHipError) as e:
        ix.encode_nodes(None, out_cap=need - 1)
    assert e.value.status == INVALID_ARGUMENT
    assert ix.encode_nodes(None, out_cap=need) == ident
    still_serves()
    # NULL offsets
    L = _lib.lib()
    assert L.ah_index_encode_nodes(ix._h, None, 0, None, 0, None, 0, None, None) == INVALID_ARGUMENT
    assert b"out_value_offsets is NULL" in L.ah_last_error()
    # a suspended index
    ix.suspend()
    try:
        status, err, _ends = raw_call(ix, None, nn)
        assert status == INVALID_ARGUMENT and "suspended" in err
    finally:
        ix.resume()
    assert ix.encode_nodes(None) == ident
    still_serves()


def test_a_listed_free_slot_is_refused():
    ds, _vecs = make(D.Euclidean, 600, 8, seed=12)
    forest = ds.build_forest([1], split_after=8)
    ix = Index(ds, forest)
    forest.close()
    delta = ix.delete_items(np.arange(0, 600, 2, dtype=np.uint32), 8)
    free = int(delta["removed"][0])
    live = int(delta["put_index"][0])
    out = np.full(4096, 0xA5, dtype=np.uint8)
    status, err, _ends = raw_call(ix, [live, live, free, 0xFFFFFFF0], 4, out=out, cap=out.size)
    assert status == INVALID_ARGUMENT and f"node_indices[2] = {free} is a free slot" in err and bool(np.all(out == 0xA5))
    with pytest.raises(_lib.ArroyHipError):
        ix.encode_nodes([free])
    assert ix.encode_nodes(None)[free] == b""  # every slot: an empty value
    assert ix.encode_nodes([live]) == [reference(ix)[live]]
    ix.close()
    ds.close()


def test_a_child_that_is_a_free_slot_is_refused():
    """A view may hold nodes no root reaches, and such a split node may name nodes of a real tree: roots 0 and 1 are Descendants
    nodes, the unreached node 2 is split(0, 1).  Dropping the first tree frees slot 0 and leaves node 2 with a free child."""
    n = 20
    ds, vecs = make(D.Euclidean, n, 8, seed=13)
    store = I.TreeStore()
    ids = np.arange(n, dtype=np.uint32)
    store.nodes = {0: ("D", ids.copy()), 1: ("D", ids.copy()), 2: ("S", 0, 1, np.zeros(1, np.float32), None)}
    store.roots = [0, 1]
    view, keep = store.to_view(D.Euclidean, 8)
    ix = Index(ds, None, view=view)
    whole = assert_whole_index(ix)
    assert whole[2] == node_codec.encode_split(0, 1, None)
    delta = ix.drop_trees(1)
    assert delta["removed"].tolist() == [0] and delta["roots"].tolist() == [1]
    queries = vecs[:4] + np.float32(1e-3)
    served = ix.search(5, queries=queries, search_k=50, raw=True)
    for indices, count in (([2], 1), ([1, 2, 2], 3), (None, 3)):
        out = np.full(256, 0xA5, dtype=np.uint8)
        status, err, _ends = raw_call(ix, indices, count, out=out, cap=out.size)
        assert status == INVALID_ARGUMENT and "has a child that is a free slot" in err and "node 2" in err, (indices, status, err)
        assert bool(np.all(out == 0xA5)), "a refused call wrote into out_values"
        again = ix.search(5, queries=queries, search_k=50, raw=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, served))
    with pytest.raises(_lib.ArroyHipError) as e:
        ix.encode_nodes(None)
    assert e.value.status == INVALID_ARGUMENT
    assert ix.encode_nodes([1]) == [node_codec.encode_descendants(ids)]  # the nodes that are whole still encode
    del keep
    ix.close()
    ds.close()


def test_encode_survives_every_allocation_failure(world):
    _ds, ix, ident, queries = world
    order = np.arange(len(ident), dtype=np.uint32)[::-1].copy()
    table = np.arange(len(ident), dtype=np.uint32)
    seen = sweep(lambda: ix.encode_nodes(order, node_ids=table))
    assert len(seen) >= 7 and all(s in (OOM, DEVICE) for s in seen) and OOM in seen, seen  # list, table, nodes, offsets, info, sums, ctl, out
    assert ix.encode_nodes(order, node_ids=table) == ident[::-1]
    assert ix.search(5, queries=queries, search_k=200)  # the index serves


# ---- 7. the Writer mirror ----------------------------------------------------------------------------------------------------
def store_values(trees, dist):
    hs = dist.header_size()
    out = {}
    for nid, nd in trees.nodes.items():
        if nd[0] == "D":
            out[nid] = node_codec.encode_descendants(nd[1])
        else:
            normal = None if nd[4] is None else np.asarray(nd[3], np.float32).tobytes().ljust(hs, b"\0")[:hs] + bytes(nd[4])
            out[nid] = node_codec.encode_split(nd[1], nd[2], normal)
    return out


@pytest.mark.parametrize("dist_name", ["Euclidean", "BinaryQuantizedCosine"])
def test_writer_mirrors_its_store_in_encoded_values(dist_name):
    """The incremental sequence of tests/test_gpu_index_insert.py (add / replace / delete, delete only, replace only, two more
    trees, three trees fewer, delete) with encoded_store set."""
    dist = getattr(D, dist_name)
    dims, n0 = 24, 900
    vecs = np.random.default_rng(5).standard_normal((n0 + 800, dims)).astype(np.float32)
    db = I.Database(dist)
    w = I.Writer(db, 0, dims)
    st = w._st
    store = {}
    followed = []

    def build(k, n_trees=5):
        b = w.builder(random.Random(40 + k)).n_trees(n_trees)
        b.encoded_store = store
        inserts, encoded = st.device_inserts, st.device_encoded_nodes
        b.build()
        want = store_values(st.trees, dist)
        assert store.keys() == want.keys(), k
        bad = [nid for nid in want if store[nid] != want[nid]]
        assert not bad, (k, len(bad), bad[:5])
        if st.device_inserts > inserts:  # the resident index followed: only what changed was encoded
            followed.append(k)
            assert 0 < st.device_encoded_nodes - encoded < len(st.trees.nodes), (k, st.device_encoded_nodes - encoded)
        else:
            assert st.device_encoded_nodes == encoded
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
    for i in range(400, 500):
        w.add_item(i, vecs[n0 + 400 + i - 400])
    build(3)
    for i in range(n0 + 300, n0 + 330):
        w.add_item(i, vecs[i])
    build(4, n_trees=7)
    for i in range(n0 + 330, n0 + 360):
        w.add_item(i, vecs[i])
    build(5, n_trees=4)
    for i in range(500, 520):
        assert w.del_item(i)
    build(6, n_trees=4)
    assert followed == [1, 2, 3, 4, 6]
    # the store opens as the index that serves: the same answers, bit for bit
    nids = sorted(store)
    opened = Index.from_encoded(st.dataset, nids, [store[nid] for nid in nids], st.trees.roots)
    qs = vecs[[1, 500, 950, 1300]]
    a, b = st.index.search(10, queries=qs, search_k=300, raw=True), opened.search(10, queries=qs, search_k=300, raw=True)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    opened.close()
    st.index.close()
    st.dataset.close()
