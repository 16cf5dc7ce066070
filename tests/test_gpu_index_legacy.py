"""ah_index_create_from_legacy (arroy_amd/csrc/index_decode.hip behind a layout): a resident index from the v0.4 - v0.6 node
bytes, upgraded.  The yardstick everywhere is array-for-array equality — ah_index_export, ah_index_export_info,
ah_index_footprint_get — with the index the existing v0.7 path (ah_index_create_from_encoded) makes of the values a host
restatement of the upgrade produces (node_codec.upgrade_values)."""
import ctypes as C
import mmap
import os
import struct

import numpy as np
import pytest

import node_legacy_cases as legacy_cases
from conftest import ROOT
from test_gpu_faults import DEVICE, OOM, sweep
from test_gpu_index_open import BASE, assert_same_index, make, spread
from test_gpu_staging import lmdb_item_offsets

pytestmark = pytest.mark.gpu

from arroy_amd import Dataset, Index, _lib, node_codec, upgrade  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from arroy_amd.index import Database, Reader  # noqa: E402

INVALID_ARGUMENT = 5
LEGACY_KEYS = ("split_values", "zero_normals", "headers_made", "item_children", "new_nodes")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"


def upgraded_index(ds, layout, node_ids, values, roots):
    up_ids, up_values, put = node_codec.upgrade_values(layout, node_ids, values, ds.distance, ds.dimensions)
    return Index.from_encoded(ds, up_ids, up_values, roots), up_ids, up_values, put


# ---- 1. the reference's own upgrade tests through the device -------------------------------------------------------------------
def stage_fixture_items(name):
    """The items of a fixture staged from pointers into the mapped file (what a reader gets from LMDB)."""
    path, dims = legacy_cases.FIXTURES[name]
    with open(os.path.join(ROOT, "tests", "golden", path), "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_COPY)
    items = lmdb_item_offsets(bytes(mm))
    rec_len = 1 + 4 + 4 * dims
    assert all(l == rec_len for _, _, l in items)
    base = C.addressof(C.c_char.from_buffer(mm))
    ds = Dataset(D.Euclidean, dims, len(items))
    ds.upload_record_pointers([i for i, _, _ in items], [base + off for _, off, _ in items], rec_len)
    ds.finalize()
    del base
    mm.close()
    return ds


@pytest.mark.parametrize("name", ["smol", "large"])
def test_the_reference_upgrade_tests_through_the_device(name, golden):
    dims, item_ids, vectors, node_ids, values, roots = legacy_cases.fixture(name)
    ds = stage_fixture_items(name)
    ix, stats, legacy = Index.from_encoded(ds, node_ids, values, roots, want_stats=True, layout="v0.6")
    ref, up_ids, up_values, put = upgraded_index(ds, "v0.6", node_ids, values, roots)
    assert_same_index(ix, ref)
    audit = ix.audit(trees=True)
    assert audit["valid"] == 1 and audit["nodes_reached"] == len(up_ids), audit
    if name == "smol":
        (tree,) = audit["tree_stats"]
        assert (tree["split_nodes"], tree["dummy_normals"], tree["descendants"], tree["depth"]) == (3, 2, 4, 4)
        assert legacy == dict(split_values=3, zero_normals=2, headers_made=1, item_children=2, new_nodes=2)
        assert ix.export_info()["n_nodes"] == 7 and ix.export()["descendants"].tolist() == [1, 5, 3, 4, 0, 2]
    else:
        assert legacy == dict(split_values=49, zero_normals=0, headers_made=49, item_children=0, new_nodes=0)
        assert ix.export_info()["n_nodes"] == 108
    assert stats["values"] == len(values) and stats["split_values"] == legacy["split_values"]
    # Reader::open on the old file, and the searches src/tests/upgrade.rs asserts
    db = Database(D.Euclidean)
    db.attach_stored(0, ds, dict(zip(item_ids, vectors)), roots, node_ids, values)
    reader = Reader.open(db, 0, version="v0.6")
    assert reader.n_items() == len(item_ids) and reader.n_trees() == len(roots) and reader.dimensions() == dims
    reader.assert_validity()
    if name == "smol":
        assert reader.stats() == {"leaf": 6, "tree_stats": [{"depth": 4, "dummy_normals": 2, "split_nodes": 3, "descendants": 4}]}
        assert reader.nns(3).search_k(100).by_vector([1.0, 0.0]) == [(1, 0.0), (0, 1.0), (2, 1.0)]
        assert ix.search(3, queries=np.array([[1.0, 0.0]], np.float32), search_k=100) == [[(1, 0.0), (0, 1.0), (2, 1.0)]]
    else:
        from test_oracle_golden import rust_display_f32
        g = golden["large_v0_6"]
        got = reader.nns(3).search_k(100).by_vector([0.0] * 30)
        assert [i for i, _ in got] == [92, 24, 78]
        assert [[int(i), rust_display_f32(np.float32(d))] for i, d in got] == g["expected"]
        assert ix.search(3, queries=np.zeros((1, 30), np.float32), search_k=100) == [got]
    # upgrade.rs through the device: the puts decode to the dump the reference asserts
    ix2, puts = upgrade.from_0_6_to_current(ds, node_ids, values, roots)
    assert_same_index(ix2, ref)
    assert [nid for nid, _ in puts] == put
    store = dict(zip(node_ids, values))
    store.update(puts)
    assert all(store[nid] == v for nid, v in zip(up_ids, up_values)), "the puts are not the upgraded values"
    want = legacy_cases.expected()[name]
    assert legacy_cases.records(D.Euclidean, dims, sorted(store), [store[k] for k in sorted(store)]) == want["trees"]
    for index in (ix, ref, ix2, db._indexes[0].index):
        index.close()
    ds.close()


# ---- 2. every metric, every legacy case, past one chunk -----------------------------------------------------------------------
PLAN = [([41, 42, 43, 44], 8), ([45], 2), ([46], 1)]  # (tree seeds, split_after): leaves of several ids, Item children, two of them
F32_METRICS = [D.Euclidean, D.Manhattan, D.Cosine, D.DotProduct]
BQ_METRICS = [D.BinaryQuantizedEuclidean, D.BinaryQuantizedManhattan, D.BinaryQuantizedCosine]
EVERY = [(m, d, 3000) for m in F32_METRICS for d in (7, 30, 100)] + [(m, d, 3000) for m in BQ_METRICS for d in (64, 200)] + [(D.Cosine, 768, 300)]


def forest_values(ds, plan=PLAN):
    """(node ids, v0.7 values, root ids) of the forest the builds of `plan` make together, the node ids spread so that ranks
    differ from ids."""
    node_ids, values, roots, at = [], [], [], 0
    for seeds, split_after in plan:
        rts, _stats, got = ds.build_forest_stream(seeds, split_after=split_after, encoded=True, node_id_base=BASE)
        nids = sorted(list(got.splits) + list(got.leaves))
        for nid in nids:
            node_ids.append(spread(at + nid))
            if nid in got.splits:
                nb, left, right = got.splits[nid][:3]
                values.append(node_codec.encode_split(spread(at + left), spread(at + right), nb))
            else:
                values.append(got.values[nid])
        roots += [spread(at + int(r) - BASE) for r in rts]
        at += max(nids) + 1
    return node_ids, values, roots


@pytest.mark.parametrize("cls,dims,n", EVERY, ids=[f"{m.__name__}-{d}" for m, d, _ in EVERY])
def test_every_metric_and_every_legacy_case_past_one_chunk(cls, dims, n):
    """A forest of 6 trees over n rows, 40 of them identical (`normal: None` nodes), rewritten into both old numberings and
    opened in chunks of three values / launches of 64 and with default knobs: the export equals the v0.7 path on
    upgrade_values(...), the stats equal the counts folded, and 64 searches equal those on the index of the upgraded values.
    Against the ORIGINAL build the searches are compared where nothing the rewriting changes can show: the two Cosine metrics
    (no header enters a margin there, and the old layout drops the headers: a Euclidean bias becomes 0) with a search_k that
    drains every tree, so that the renumbered one-id nodes cannot change which candidates a tie of the queue lets through."""
    ds, vecs = make(cls, n, dims, seed=dims + cls.metric, duplicates=40)
    node_ids, values, roots = forest_values(ds)
    original = Index.from_encoded(ds, node_ids, values, roots)
    queries = vecs[np.arange(64) * 37 % n] + np.float32(1e-3)
    everything = len(roots) * n  # a search_k that visits every leaf: no tie of the queue can change the candidates
    for layout in ("v0.5", "v0.4"):
        old_ids, old_values, counts = legacy_cases.fold_to_legacy(layout, node_ids, values, cls, dims)
        # every case is there (counted on the CPU before anything is opened)
        assert counts["left_items"] - counts["both_items"] > 0 and counts["right_items"] - counts["both_items"] > 0, counts
        assert counts["both_items"] > 0 and counts["zero_normals"] > 0 and counts["headers_made"] > 0, counts
        assert cls.binary_quantized or counts["minus_zero"] > 0, counts
        assert any(v[0] == 1 for v in old_values) and len(old_values) > (1000 if n == 3000 else 100)
        ref, up_ids, up_values, _put = upgraded_index(ds, layout, old_ids, old_values, roots)
        assert len(up_ids) == len(old_ids) + counts["new_nodes"] == len(node_ids)
        largest = max((len(v) + 15) & ~15 for v in old_values)
        opened = []
        for knobs in (dict(AH_DECODE_CHUNK_BYTES=3 * largest, AH_LAUNCH_MAX_ITEMS=64), dict()):
            with _lib.tuning(**knobs):
                ix, stats, legacy = Index.from_encoded(ds, old_ids, old_values, roots, want_stats=True, layout=layout)
            assert (stats["chunks"] > 10) == bool(knobs), stats
            assert_same_index(ix, ref)
            assert legacy == {k: counts[k] for k in LEGACY_KEYS}, (legacy, counts)
            opened.append(ix)
        ix = opened[0]
        audit = ix.audit()
        assert audit["valid"] == 1 and audit["nodes_reached"] == len(up_ids), audit
        ex = ix.export()
        if cls is D.Cosine:  # the headers ah_dataset_upload_vectors gives the same vectors
            rows = np.ascontiguousarray(ex["normal_rows"]).view(np.float32).reshape(len(ex["normal_rows"]), -1)[:, :dims]
            again = Dataset(cls, dims, len(rows))
            again.upload_vectors(np.arange(len(rows), dtype=np.uint32), rows)
            again.finalize()
            assert again.read_headers().astype(np.float32).tobytes() == np.ascontiguousarray(ex["normal_headers"]).tobytes()
            again.close()
        elif cls is D.BinaryQuantizedCosine:
            assert np.all(ex["normal_headers"] == np.float32(np.sqrt(np.float32(64 * ((dims + 63) // 64)))))
        else:
            assert not np.any(np.ascontiguousarray(ex["normal_headers"]).view(np.uint32)), "the other metrics get all-zero headers"
        assert ix.search(10, queries=queries, search_k=300) == ref.search(10, queries=queries, search_k=300)
        if cls in (D.Cosine, D.BinaryQuantizedCosine):  # no header enters a margin: the original build's answers
            assert ix.search(10, queries=queries, search_k=everything) == original.search(10, queries=queries, search_k=everything)
        for index in opened + [ref]:
            index.close()
    original.close()
    ds.close()


# ---- the rest on one small Euclidean forest ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good():
    ds, vecs = make(D.Euclidean, 600, 30, seed=6, duplicates=30)
    node_ids, values, roots = forest_values(ds, [([5, 6], 8), ([7], 1)])
    folded = {layout: legacy_cases.fold_to_legacy(layout, node_ids, values, D.Euclidean, 30) for layout in ("v0.5", "v0.4")}
    yield ds, vecs, node_ids, values, roots, folded
    ds.close()


def raw_call(ds, layout, node_ids, values, roots, want_legacy=True):
    """ah_index_create_from_legacy itself -> (status, handle value, decode stats, legacy stats)."""
    n = len(node_ids)
    keep = [np.frombuffer(bytes(v), np.uint8) for v in values]
    ptrs = (C.c_void_p * max(1, n))(*[a.ctypes.data for a in keep])
    lens = (C.c_size_t * max(1, n))(*[a.size for a in keep])
    ids, rts, h = np.array(node_ids, np.uint32), np.array(roots, np.uint32), C.c_void_p(99)
    st, legacy = _lib.AhIndexDecodeStats(), _lib.AhIndexLegacyStats(7, 7, 7, 7, 7)
    status = _lib.lib().ah_index_create_from_legacy(ds._h, layout, ids.ctypes.data, ptrs, lens, n, rts.ctypes.data, len(roots), C.byref(h),
                                                    C.byref(st), C.byref(legacy) if want_legacy else None)
    return status, h, st, legacy


def test_layout_0_7_through_the_new_call_is_the_existing_open(good):
    ds, _vecs, node_ids, values, roots, _folded = good
    want, want_stats = Index.from_encoded(ds, node_ids, values, roots, want_stats=True)
    status, h, st, legacy = raw_call(ds, _lib.NODE_LAYOUT_V0_7, node_ids, values, roots)
    assert status == 0 and h.value not in (None, 99)
    got = Index.__new__(Index)
    got.dataset, got._h = ds, h
    import weakref
    got._filters = weakref.WeakSet()
    assert_same_index(got, want)
    for k, _ in _lib.AhIndexDecodeStats._fields_:
        if not k.startswith("seconds"):
            assert int(getattr(st, k)) == want_stats[k], k
    assert [int(getattr(legacy, k)) for k in LEGACY_KEYS] == [0] * 5
    # ... and the legacy values are refused by the v0.7 layout, as by ah_index_create_from_encoded
    old_ids, old_values, _counts = _folded["v0.5"]
    status, h2, _st, _legacy = raw_call(ds, _lib.NODE_LAYOUT_V0_7, old_ids, old_values, roots)
    assert status == INVALID_ARGUMENT and h2.value is None and b"split value" in _lib.lib().ah_last_error()
    got.close(), want.close()


def refused(ds, layout, node_ids, values, roots):
    with pytest.raises(_lib.ArroyHipError) as e:
        Index.from_encoded(ds, node_ids, values, roots, layout=layout)
    assert e.value.status == INVALID_ARGUMENT, str(e.value)
    return str(e.value)


def test_malformed_legacy_values_are_refused_by_name(good):
    ds, vecs, _node_ids, v07_values, roots, folded = good
    hs, vs = 4, 120
    live_before = None
    for layout, wrong_modes in (("v0.5", (0, 1)), ("v0.4", (2, 3))):
        node_ids, values, _counts = folded[layout]
        Index.from_encoded(ds, node_ids, values, roots, layout=layout).close()
        if live_before is None:
            live_before = _lib.device_cache_stats(0)[0]
        modes = node_codec.legacy_modes(layout)
        splits = [i for i, v in enumerate(values) if v[0] == 2]
        leaves = [i for i, v in enumerate(values) if v[0] == 1]
        tree_left = [i for i in splits if values[i][1] == modes["tree"]]
        at = tree_left[len(tree_left) // 3]
        assert min(leaves) < at < max(leaves)
        v = values[at]
        v07 = next(x for x in v07_values if len(x) == 9 + hs + vs)
        cases = {
            "split_of_9_bytes": (v[:9], "11 + vector"),
            "split_in_the_v0_7_layout": (v07, "11 + vector"),
            "split_one_short": (v[:-1], "11 + vector"),
            f"left_mode_{wrong_modes[0]}": (v[:1] + bytes([wrong_modes[0]]) + v[2:], "mode byte"),
            f"right_mode_{wrong_modes[1]}": (v[:6] + bytes([wrong_modes[1]]) + v[7:], "mode byte"),
            "left_mode_9": (v[:1] + b"\x09" + v[2:], "mode byte"),
            "tree_child_absent": (v[:2] + struct.pack(">I", 5) + v[6:], "child id"),
            "tag_7": (b"\7" + v[1:], "unknown node tag"),
        }
        assert len(v07) == 9 + hs + vs != 11 + vs
        for name, (bad_value, words) in cases.items():
            bad = list(values)
            bad[at] = bad_value
            msg = refused(ds, layout, node_ids, bad, roots)
            assert f"node {node_ids[at]} " in msg and words in msg, (layout, name, msg)
            # two bad values: the smaller position is named, whichever pass finds which
            later = max(i for i in splits if i > at)
            bad[later] = values[later][:1] + b"\x09" + values[later][2:]
            msg = refused(ds, layout, node_ids, bad, roots)
            assert f"node {node_ids[at]} " in msg and words in msg, (layout, name, "with a bad mode behind it", msg)
            earlier = min(i for i in splits if i < at)
            bad[earlier] = values[earlier][:-1]
            msg = refused(ds, layout, node_ids, bad, roots)
            assert f"node {node_ids[earlier]} " in msg and "11 + vector" in msg, (layout, name, "with a short split in front of it", msg)
        msg = refused(ds, layout, node_ids, values, roots[:-1] + [5])
        assert "root 2 (node 5)" in msg and "root id" in msg, msg
        # an Item child is no node id: the same number as an absent Tree child is fine as an item
        item_left = [i for i in splits if values[i][1] == modes["item"]]
        assert item_left
    with pytest.raises(ValueError):
        Index.from_encoded(ds, node_ids, values, roots, layout="v0.3")
    status, h, _st, _legacy = raw_call(ds, 3, node_ids, values, roots)
    assert status == INVALID_ARGUMENT and h.value is None and b"unknown node layout" in _lib.lib().ah_last_error()
    assert _lib.device_cache_stats(0)[0] == live_before, "a refused call holds device memory"
    ds.update_vectors([], [599], vecs[599:600])  # no index of the dataset is left


def test_every_allocation_of_the_legacy_call_may_fail(good):
    ds, _vecs, _node_ids, _values, roots, folded = good
    node_ids, values, counts = folded["v0.5"]
    assert counts["new_nodes"] > 40
    ref, _ids, _values, _put = upgraded_index(ds, "v0.5", node_ids, values, roots)
    largest = max((len(v) + 15) & ~15 for v in values)
    with _lib.tuning(AH_DECODE_CHUNK_BYTES=40 * largest):  # a few chunks: the arrays and the new nodes' ids grow between them
        seen = sweep(lambda: Index.from_encoded(ds, node_ids, values, roots, layout="v0.5"), cleanup=lambda ix: ix.close())
        assert len(seen) >= 10 and OOM in seen and all(s in (OOM, DEVICE) for s in seen), seen
        for nth in (1, len(seen)):  # the first and the last allocation: *out is NULL, the stats untouched by a result
            _lib.tuning_set("AH_FAIL_ALLOC_AFTER", nth)
            try:
                status, h, _st, legacy = raw_call(ds, _lib.NODE_LAYOUT_V0_5, node_ids, values, roots)
            finally:
                _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
            assert status in (OOM, DEVICE) and h.value is None and legacy.new_nodes == 0, (nth, status)
        ix = Index.from_encoded(ds, node_ids, values, roots, layout="v0.5")
    assert_same_index(ix, ref)
    ix.close(), ref.close()


def test_the_v0_4_upgrade_renumbers_the_modes_and_opens_the_same_index(good):
    """upgrade.cosine_from_0_4_to_0_5: the puts are the values in the v0.5 numbering — what the rewriting of the same forest
    into that numbering gives — and the index is the one either numbering opens."""
    ds, _vecs, _node_ids, _values, roots, folded = good
    ids4, values4, _counts = folded["v0.4"]
    ids5, values5, _counts = folded["v0.5"]
    assert ids4 == ids5 and values4 != values5
    ix, puts = upgrade.cosine_from_0_4_to_0_5(ds, ids4, values4, roots)
    assert [nid for nid, _ in puts] == ids5 and [v for _, v in puts] == values5
    ref = Index.from_encoded(ds, ids5, values5, roots, layout="v0.5")
    assert_same_index(ix, ref)
    ix2, puts7 = upgrade.from_0_6_to_current(ds, ids5, [v for _, v in puts], roots)
    assert_same_index(ix2, ref)
    up_ids, up_values, put = node_codec.upgrade_values("v0.5", ids5, values5, D.Euclidean, 30)
    assert [nid for nid, _ in puts7] == put and dict(puts7) == {n: v for n, v in zip(up_ids, up_values) if n in set(put)}
    ix.close(), ix2.close(), ref.close()


def test_maintenance_of_an_opened_legacy_index(good):
    ds, vecs, _node_ids, _values, roots, folded = good
    node_ids, values, _counts = folded["v0.4"]
    ix = Index.from_encoded(ds, node_ids, values, roots, layout="v0.4")
    ref, _ids, _values, _put = upgraded_index(ds, "v0.4", node_ids, values, roots)
    assert_same_index(ix, ref)
    queries = vecs[np.arange(16) * 31 % 600] + np.float32(1e-3)
    gone = np.arange(3, 600, 5, dtype=np.uint32)
    da, db = ix.delete_items(gone, 20), ref.delete_items(gone, 20)
    assert da.keys() == db.keys() and all(da[k].tobytes() == db[k].tobytes() for k in da)
    assert_same_index(ix, ref)
    assert ix.compact() == ref.compact()
    assert_same_index(ix, ref)
    assert ix.audit()["bad_link"] == 0 and ix.footprint()["free_slots"] == 0
    keep = np.arange(0, 600, 3, dtype=np.uint32)
    fa, fb = ix.make_filter(keep, sorted=True), ref.make_filter(keep, sorted=True)
    got = ix.search(10, queries=queries, search_k=300, candidates=fa)
    assert got == ref.search(10, queries=queries, search_k=300, candidates=fb)
    assert all(i % 3 == 0 and i not in set(gone.tolist()) for res in got for i, _ in res)
    fa.close(), fb.close()
    # ... and the write-back of the maintained index: v0.7 values under the store's ids
    id_of = np.arange(ix.export_info()["n_nodes"], dtype=np.uint32) + np.uint32(1000)
    assert ix.encode_nodes(None, node_ids=id_of) == ref.encode_nodes(None, node_ids=id_of)
    ix.close(), ref.close()
