"""The hand-over of the arrays of a resident index from one maintenance call to the next: delete -> insert -> graft (past
normals_cap, so the normal rows move into larger arrays) -> compact, on ONE index, on a binary-quantized metric and an f32 one.
After every step the index must audit valid, its export must make (ah_index_create_from_view) an index that holds the same
forest, and the searches of the live index and of that fresh one must agree in ids and distance bits.  What a call leaves
dangling (a normals view that still names the arrays it freed, a stale rank array, a count that was not carried over) shows
here at the latest one step later."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

from arroy_amd import Dataset, Index  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from arroy_amd.index import TreeStore  # noqa: E402

N, DIMS, SPLIT_AFTER = 300, 64, 8
SEEDS = [11, 12, 13]
NONE = 0xFFFFFFFF


def store_of_export(ex, dist):
    """The export as a TreeStore keyed by node slot: free slots (kind 0) are left out, a split node's plane is its normal ROW
    (the first vector_size bytes of it: the rest is the zero fill of the device pitch) and header."""
    vs, hs = dist.vector_size(DIMS), dist.header_size()
    s = TreeStore()
    desc = ex["descendants"]
    for i, nd in enumerate(ex["nodes"]):
        if nd["kind"] == 1:
            s.nodes[i] = ("D", desc[int(nd["offset"]):int(nd["offset"]) + int(nd["count"])].copy())
        elif nd["kind"] == 2:
            row = int(nd["offset"])
            has = bool(nd["has_normal"])
            s.nodes[i] = ("S", int(nd["left"]), int(nd["right"]), ex["normal_headers"][row].copy() if has else np.zeros(hs // 4, np.float32),
                          ex["normal_rows"][row, :vs].tobytes() if has else None)
        else:
            assert nd["kind"] == 0
    s.roots = [int(r) for r in ex["roots"]]
    return s


def same_forest(a, da, b, db, dist):
    """export `a` (slot -> node id: da) holds the forest of export `b` (db): node for node, id for id, row bits for row bits"""
    sa, sb = store_of_export(a, dist), store_of_export(b, dist)
    assert sorted(da[i] for i in sa.nodes) == sorted(db[i] for i in sb.nodes)
    assert [da[r] for r in sa.roots] == [db[r] for r in sb.roots]
    back = {db[i]: i for i in sb.nodes}
    for i, x in sa.nodes.items():
        y = sb.nodes[back[da[i]]]
        assert x[0] == y[0], i
        if x[0] == "D":
            assert np.array_equal(x[1], y[1]), i
        else:
            assert (da[x[1]], da[x[2]]) == (db[y[1]], db[y[2]]), i
            assert x[4] == y[4] and (x[4] is None or x[3].tobytes() == y[3].tobytes()), i


def check(ds, ix, dist, queries, step, byte_for_byte=False):
    rep = ix.audit()
    assert rep["valid"], (step, rep)
    ex = ix.export()
    store = store_of_export(ex, dist)
    view, keep = store.to_view(dist, DIMS)
    fresh = Index(ds, None, view=view)
    try:
        assert fresh.audit()["valid"], step
        back = ix.export()  # (a second export of the live index: the first one did not disturb it)
        fx = fresh.export()
        same_forest(back, {i: i for i in range(back["nodes"].size)}, fx, {d: nid for nid, d in keep[4].items()}, dist)
        if byte_for_byte:  # after a compaction the index IS the fresh one
            for key in ("nodes", "roots", "descendants", "normal_rows", "normal_headers"):
                assert ex[key].shape == fx[key].shape and ex[key].tobytes() == fx[key].tobytes(), (step, key)
            assert ix.export_info() == fresh.export_info() and ix.footprint() == fresh.footprint(), step
        for sk in (40, 10 ** 9):  # (the second opens every leaf)
            x = ix.search(10, queries=queries, search_k=sk, raw=True)
            y = fresh.search(10, queries=queries, search_k=sk, raw=True)
            assert np.array_equal(x[2], y[2]) and np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes(), (step, sk)
    finally:
        fresh.close()
    return ex


def rebuilt_subtree(ex, dist, seed):
    """-> (view, keepalive, target): the largest Descendants node of the export as a sub-tree of two split nodes with a plane
    each over the same ids, so that every tree still holds every item once"""
    g = np.random.default_rng(seed)
    nodes = ex["nodes"]
    leaves = np.flatnonzero(nodes["kind"] == 1)
    target = int(leaves[np.argmax(nodes["count"][leaves])])
    ids = ex["descendants"][int(nodes["offset"][target]):int(nodes["offset"][target]) + int(nodes["count"][target])]
    assert ids.size >= 3
    vs, hs = dist.vector_size(DIMS), dist.header_size()

    def plane():
        if dist.binary_quantized:
            return g.integers(0, 256, vs, dtype=np.uint8).tobytes()
        return g.standard_normal(vs // 4).astype(np.float32).tobytes()
    third = ids.size // 3
    sub = TreeStore()
    sub.nodes[0] = ("D", ids[:third].copy())
    sub.nodes[1] = ("D", ids[third:2 * third].copy())
    sub.nodes[2] = ("D", ids[2 * third:].copy())
    sub.nodes[3] = ("S", 0, 1, g.standard_normal(hs // 4).astype(np.float32), plane())
    sub.nodes[4] = ("S", 3, 2, g.standard_normal(hs // 4).astype(np.float32), plane())
    sub.roots = [4]
    view, keep = sub.to_view(dist, DIMS)
    return view, keep, target


@pytest.mark.parametrize("dist", [D.BinaryQuantizedCosine, D.Cosine], ids=lambda d: d.__name__)
def test_delete_insert_graft_compact_hand_the_arrays_over(dist):
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    vecs = O.synth(5, 1, N, DIMS)
    ids = np.arange(N, dtype=np.uint32)
    ds = Dataset(dist, DIMS, N)
    ds.upload_vectors(ids, vecs)
    ds.finalize()
    queries = vecs[np.random.default_rng(9).integers(0, N, 8)] + np.float32(1e-3)
    forest = ds.build_forest(SEEDS, split_after=SPLIT_AFTER)
    ix = Index(ds, forest)
    forest.close()
    try:
        start = check(ds, ix, dist, queries, "fresh")
        n_normals = ix.export_info()["n_normals"]
        assert n_normals >= 3 and ix.footprint()["normals_cap"] == n_normals
        # 1. delete a tenth of the items
        gone = np.sort(np.random.default_rng(2).permutation(ids)[:N // 10])
        delta = ix.delete_items(gone, SPLIT_AFTER)
        assert delta["removed"].size > 0  # (free slots and orphaned rows from here on)
        ix.suspend()  # the items leave the dataset as well, as in an incremental build: the audit asks for every row in every tree
        ds.update_vectors(gone, np.zeros(0, np.uint32), np.zeros((0, DIMS), np.float32))
        ix.resume()
        ex = check(ds, ix, dist, queries, "delete")
        assert not np.isin(gone, ex["descendants"]).any() and ex["descendants"].size == 3 * (N - gone.size)
        # 2. insert them back
        ix.suspend()
        ds.update_vectors(np.zeros(0, np.uint32), gone, vecs[gone])
        ix.resume()
        delta = ix.insert_items(gone, SEEDS)
        assert delta["put_index"].size > 0
        ex = check(ds, ix, dist, queries, "insert")
        assert ex["descendants"].size == 3 * N == start["descendants"].size
        # 3. graft a rebuilt sub-tree: two planes more than the rows have room for
        fp = ix.footprint()
        assert fp["normals_cap"] == fp["n_normals"] == n_normals and fp["free_slots"] > 0
        view, keep, target = rebuilt_subtree(ex, dist, 17)
        m = ix.graft(view, np.array([target], dtype=np.uint32), None, want_map=True)
        assert m.size == ex["nodes"].size and (m == NONE).sum() == fp["free_slots"]
        fp2 = ix.footprint()
        assert fp2["n_normals"] == n_normals + 2 and fp2["normals_cap"] >= 2 * n_normals and fp2["free_slots"] == 0
        assert fp2["live_normals"] < fp2["n_normals"]  # (the rows the delete orphaned are still there)
        ex = check(ds, ix, dist, queries, "graft")
        assert ex["descendants"].size == 3 * N
        # 4. compact
        stats = ix.compact()
        assert stats["moved"] == 1 and stats["normals_after"] == stats["normals_cap_after"] == fp2["live_normals"]
        ex = check(ds, ix, dist, queries, "compact", byte_for_byte=True)
        assert ex["nodes"].size == fp2["n_nodes"] and ex["normal_rows"].shape[0] == fp2["live_normals"]
    finally:
        ix.close()
        ds.close()
