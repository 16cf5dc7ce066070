"""ah_index_create_from_encoded (arroy_amd/csrc/index_decode.hip): a resident index from the `NodeCodec` values LMDB stores.
The yardstick everywhere is array-for-array equality — ah_index_export, ah_index_export_info, ah_index_footprint_get — with the
index ah_index_create_from_view makes of the view decoded in Python (arroy_amd/node_codec.py, arroy_amd/roaring.py) with
children and roots replaced by their ranks among the node ids."""
import struct

import numpy as np
import pytest

import node_codec_cases as cases
from test_gpu_faults import DEVICE, OOM, sweep

pytestmark = pytest.mark.gpu

import ctypes as C  # noqa: E402

from arroy_amd import Dataset, Index, _lib, node_codec, roaring  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from arroy_amd.dataset import _NODE_DT  # noqa: E402

INVALID_ARGUMENT = 5
BASE = 0x01020304
METRICS = [D.Euclidean, D.Manhattan, D.Cosine, D.DotProduct, D.BinaryQuantizedEuclidean, D.BinaryQuantizedManhattan,
           D.BinaryQuantizedCosine]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"


def make(cls, n, dims, seed, duplicates=0):
    vecs = np.random.default_rng(seed).standard_normal((n, dims)).astype(np.float32)
    if duplicates:
        vecs[100:100 + duplicates] = vecs[100]  # identical rows: nodes over them have `normal: None`
    ds = Dataset(cls, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    if cls.metric == 3:
        ds.preprocess_dot()
    ds.finalize()
    return ds, vecs


def spread(nid: int) -> int:
    """Every other node id shifted further: strictly increasing, and no id is its own rank."""
    return BASE + nid + 3 * (nid // 2)


def stream_values(ds, seeds, split_after):
    """(node_ids, values, root ids) of an encoded build, the node ids spread so that ranks differ from ids."""
    roots, _stats, got = ds.build_forest_stream(seeds, split_after=split_after, encoded=True, node_id_base=BASE)
    nids = sorted(list(got.splits) + list(got.leaves))
    values = []
    for nid in nids:
        if nid in got.splits:
            nb, left, right = got.splits[nid][:3]
            values.append(node_codec.encode_split(spread(left), spread(right), nb))
        else:
            values.append(got.values[nid])
    return [spread(n) for n in nids], values, [spread(int(r) - BASE) for r in roots]


def decoded(dist, dims, values):
    return [node_codec.decode_value(dist, dims, v) for v in values]


def reference_index(ds, node_ids, nodes_decoded, roots):
    """The index ah_index_create_from_view makes of the decoded view: ranks for ids, descendants and normals in node order."""
    dist, dims = ds.distance, ds.dimensions
    rank = {int(x): i for i, x in enumerate(node_ids)}
    stride = dist.header_size() + dist.vector_size(dims)
    nodes = np.zeros(max(1, len(node_ids)), dtype=_NODE_DT)
    desc, normals = [], []
    at = 0
    for i, dec in enumerate(nodes_decoded):
        if dec[0] == "S":
            nodes["kind"][i], nodes["left"][i], nodes["right"][i] = 2, rank[dec[1]], rank[dec[2]]
            if dec[3] is not None:
                nodes["has_normal"][i], nodes["offset"][i] = 1, len(normals) * stride
                normals.append(bytes(dec[3]))
        else:
            nodes["kind"][i], nodes["offset"][i], nodes["count"][i] = 1, at, dec[1].size
            desc.append(np.asarray(dec[1], np.uint32))
            at += dec[1].size
    desc = np.concatenate(desc).astype(np.uint32) if desc else np.zeros(0, np.uint32)
    blob = np.frombuffer(b"".join(normals) or b"\0", dtype=np.uint8)
    rts = np.array([rank[int(r)] for r in roots] or [0], dtype=np.uint32)
    keep_desc = desc if desc.size else np.zeros(1, np.uint32)
    v = _lib.AhForestView()
    v.n_trees, v.n_nodes = len(roots), len(node_ids)
    v.roots = rts.ctypes.data_as(C.POINTER(C.c_uint32))
    v.nodes = C.cast(nodes.ctypes.data, C.POINTER(_lib.AhNode))
    v.normals = blob.ctypes.data_as(C.POINTER(C.c_uint8))
    v.normals_len = len(normals) * stride
    v.normal_stride, v.normal_vector_offset, v.normal_header_offset = stride, dist.header_size(), 0
    v.descendants = keep_desc.ctypes.data_as(C.POINTER(C.c_uint32))
    v.descendants_len = desc.size
    return Index(ds, None, view=v)


def assert_same_index(got, want):
    assert got.export_info() == want.export_info()
    assert got.footprint() == want.footprint()
    a, b = got.export(), want.export()
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def check(ds, node_ids, values, roots, nodes_decoded=None):
    """from_encoded against the reference; returns (index, reference index, stats)."""
    ix, stats = Index.from_encoded(ds, node_ids, values, roots, want_stats=True)
    ref = reference_index(ds, node_ids, decoded(ds.distance, ds.dimensions, values) if nodes_decoded is None else nodes_decoded, roots)
    assert_same_index(ix, ref)
    return ix, ref, stats


# ---- round trip ---------------------------------------------------------------------------------------------------------------
ROUND_TRIP = [(m, dims) for m in METRICS for dims in (30, 70)]


@pytest.mark.parametrize("cls,dims", ROUND_TRIP, ids=[f"{m.__name__}-{d}" for m, d in ROUND_TRIP])
def test_round_trip_of_an_encoded_build(cls, dims):
    """900 rows, 40 of them identical, 3 trees with leaves of at most 16 ids: dims 30 pads the f32 pitch, dims 70 gives the
    1-bit rows a second 64-bit word."""
    ds, vecs = make(cls, 900, dims, seed=dims + cls.metric, duplicates=40)
    node_ids, values, roots = stream_values(ds, [41, 42, 43], split_after=16)
    assert all(i != nid for i, nid in enumerate(node_ids))
    ix, ref, stats = check(ds, node_ids, values, roots)
    n_split = sum(v[0] == 2 for v in values)
    assert any(len(v) == 9 for v in values), "no `normal: None` value in the build"
    assert stats["values"] == len(values) and stats["split_values"] == n_split and stats["descendants_values"] == len(values) - n_split
    assert stats["normals"] == sum(len(v) > 9 for v in values if v[0] == 2) and stats["ids"] == 3 * 900 and stats["chunks"] == 1
    assert stats["wave_values"] == len(values) - n_split and stats["block_containers"] == 0
    queries = vecs[np.arange(32) * 27 % 900] + np.float32(1e-3)
    for index in (ix, ref):
        index.keep = index.make_filter(np.arange(0, 900, 3, dtype=np.uint32), sorted=True)
    assert ix.search(10, queries=queries, search_k=300) == ref.search(10, queries=queries, search_k=300)
    assert ix.search(10, queries=queries, search_k=300, candidates=ix.keep) == ref.search(10, queries=queries, search_k=300, candidates=ref.keep)
    audit = ix.audit()
    assert audit["valid"] == 1 and audit["nodes_reached"] == len(values), audit
    # the same values in chunks of a few values, launches of 64: normals and lists that cross chunks
    largest = max((len(v) + 15) & ~15 for v in values)
    with _lib.tuning(AH_DECODE_CHUNK_BYTES=3 * largest, AH_LAUNCH_MAX_ITEMS=64):
        small, small_stats = Index.from_encoded(ds, node_ids, values, roots, want_stats=True)
    assert small_stats["chunks"] > 10
    assert_same_index(small, ref)
    for index in (ix, ref, small):
        index.close()
    ds.close()


def test_the_values_roaring_wrote_as_59_roots():
    values = cases.fixture_descendants()
    assert len(values) == 59
    ds, _ = make(D.Euclidean, 100, 30, seed=2)
    node_ids = [7 + 5 * i for i in range(59)]
    ix, ref, stats = check(ds, node_ids, values, node_ids)
    lists = [node_codec.decode_value(D.Euclidean, 30, v)[1] for v in values]
    assert ix.export()["descendants"].tolist() == np.concatenate(lists).tolist()
    assert stats["descendants_values"] == 59 and stats["split_values"] == 0 and stats["ids"] == sum(l.size for l in lists)
    ix.close(), ref.close(), ds.close()


# ---- every container rule in one call -------------------------------------------------------------------------------------------
def desc_value(conts, runs):
    return bytes([node_codec.TAG_DESCENDANTS]) + roaring.assemble(conts, runs)


def ids_of(conts):
    out = []
    for key, kind, card, body in conts:
        if kind == roaring.RUN:
            (n,) = struct.unpack_from("<H", body)
            pairs = np.frombuffer(body, dtype="<u2", offset=2).reshape(n, 2).astype(np.int64)
            lows = np.concatenate([np.arange(s, s + l + 1) for s, l in pairs]) if n else np.zeros(0, np.int64)
        elif kind == roaring.ARRAY:
            lows = np.frombuffer(body, dtype="<u2").astype(np.int64)
        else:
            lows = np.flatnonzero(np.unpackbits(np.frombuffer(body, dtype=np.uint8), bitorder="little"))
        assert lows.size == card
        out.append((key << 16) + lows)
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)


def edge_values():
    """[(name, value, ids, [container kinds])], ordinary array leaves between them."""
    rng = np.random.default_rng(77)
    sets = {
        "empty": np.zeros(0, np.uint32),
        "one": np.array([7], np.uint32),
        "containers_300": (np.arange(300, dtype=np.uint32) << 16) + rng.integers(0, 65536, 300).astype(np.uint32),
        "array_4096": np.arange(0, 2 * 4096, 2, dtype=np.uint32) + np.uint32(3 << 16),
        "bitmap_4097": np.arange(0, 3 * 4097, 3, dtype=np.uint32) + np.uint32(5 << 16),
        "full_key": np.arange(2 << 16, 3 << 16, dtype=np.uint32),
        "key_ffff": np.uint32(0xFFFF0000) + np.array([0, 1, 2, 700, 65535], np.uint32),
        "three_keys": np.concatenate([np.arange(10, 500) + (k << 16) for k in (1, 4, 0xFFFF)]).astype(np.uint32),
        "five_keys": np.concatenate([np.arange(k, 300 + 7 * k) + (k << 16) for k in range(5)]).astype(np.uint32),
        "bitmap_array_one": cases.edge_lists()["bitmap_array_one"],
        "wave_edges": cases.edge_lists()["wave_edges"],
    }
    out = []
    for name, ids in sets.items():
        for runs in (False, True):
            conts = roaring.containers(ids, runs)
            out.append((f"{name}-{'runs' if runs else 'plain'}", desc_value(conts, runs), ids, [k for _, k, _, _ in conts]))
    by_hand = {
        "one_run_0_65535": [(9, roaring.RUN, 65536, roaring.run_body([0], [65535]))],
        "runs_2048_of_one": [(4, roaring.RUN, 2048, roaring.run_body(np.arange(2048) * 3, np.zeros(2048, np.int64)))],
        "runs_300_in_two_rounds": [(1, roaring.ARRAY, 3, roaring.array_body([1, 2, 9])),
                                   (2, roaring.RUN, 300 * 4, roaring.run_body(np.arange(300) * 100, np.full(300, 3))),
                                   (3, roaring.BITMAP, 5000, roaring.bitmap_body(np.arange(5000) * 13)),
                                   (8, roaring.RUN, 70, roaring.run_body([5, 100], [9, 59]))],
    }
    for name, conts in by_hand.items():
        out.append((name, desc_value(conts, True), ids_of(conts), [k for _, k, _, _ in conts]))
    leaf = np.sort(rng.choice(1 << 16, size=20, replace=False)).astype(np.uint32)
    plain = ("leaf", node_codec.encode_descendants(leaf), leaf, [roaring.ARRAY])
    mixed = [plain]
    for item in out:
        mixed += [item, plain]
    return mixed


def test_every_container_rule_in_one_call():
    edge = edge_values()
    ds, _ = make(D.Euclidean, 100, 30, seed=3)
    node_ids = [11 + 3 * i for i in range(len(edge))]
    values = [v for _, v, _, _ in edge]
    ix, ref, stats = check(ds, node_ids, values, node_ids, nodes_decoded=[("D", ids) for _, _, ids, _ in edge])
    kinds = [k for _, _, _, ks in edge for k in ks]
    assert stats["containers_array"] == kinds.count(roaring.ARRAY) and stats["containers_bitmap"] == kinds.count(roaring.BITMAP)
    assert stats["containers_run"] == kinds.count(roaring.RUN) and min(kinds.count(k) for k in (0, 1, 2)) > 0
    on_block = [ks for _, _, _, ks in edge if any(k != roaring.ARRAY for k in ks)]
    assert stats["block_containers"] == sum(len(ks) for ks in on_block) > 0
    assert stats["wave_values"] == len(edge) - len(on_block) > 0
    assert stats["ids"] == sum(ids.size for _, _, ids, _ in edge)
    # ... and each value alone, whatever its path
    for (name, value, ids, _), nid in zip(edge[1::2], node_ids):
        one = Index.from_encoded(ds, [nid], [value], [nid])
        assert one.export()["descendants"].tobytes() == ids.tobytes(), name
        one.close()
    ix.close(), ref.close(), ds.close()


def greedy_chunks(values, limit):
    units = [(len(v) + 15) & ~15 for v in values]
    limit = max([limit, 16] + units)
    chunks, room = 0, 0
    for u in units:
        if chunks == 0 or u > room:
            chunks, room = chunks + 1, limit
        room -= u
    return chunks


def test_several_chunks_launches_and_scan_tiles():
    rng = np.random.default_rng(9)
    many = [np.sort(rng.choice(1 << 20, size=int(k), replace=False)).astype(np.uint32) for k in rng.integers(0, 41, size=5000)]
    values = [node_codec.encode_descendants(l) for l in many]
    node_ids = (np.arange(5000, dtype=np.uint32) * 2 + 1).tolist()
    ds, _ = make(D.Euclidean, 100, 30, seed=4)
    ref = reference_index(ds, node_ids, [("D", l) for l in many], node_ids)
    tight = max((len(v) + 15) & ~15 for v in values) + 16  # just above the largest value
    seen = []
    for knobs in (dict(AH_DECODE_CHUNK_BYTES=tight), dict(AH_LAUNCH_MAX_ITEMS=64), dict(AH_DECODE_CHUNK_BYTES=tight, AH_LAUNCH_MAX_ITEMS=64), dict()):
        with _lib.tuning(**knobs):
            ix, stats = Index.from_encoded(ds, node_ids, values, node_ids, want_stats=True)
        assert_same_index(ix, ref)
        limit = knobs.get("AH_DECODE_CHUNK_BYTES", 64 << 20)
        assert stats["chunks"] == greedy_chunks(values, limit), knobs
        seen.append(stats["chunks"])
        ix.close()
    assert seen[0] == seen[2] > 1000 and seen[1] == seen[3] == 1  # (5000 values in one chunk: two tiles of the scans)
    with _lib.tuning(AH_DECODE_CHUNK_BYTES=1):  # never below the largest value
        ix = Index.from_encoded(ds, node_ids[:50], values[:50], node_ids[:50])
    assert ix.export()["descendants"].tobytes() == np.concatenate(many[:50]).tobytes()
    ix.close(), ref.close(), ds.close()


def test_values_at_odd_addresses_and_an_empty_forest():
    ds, _ = make(D.DotProduct, 600, 30, seed=5, duplicates=30)
    node_ids, values, roots = stream_values(ds, [1, 2, 3], split_after=20)
    ref = reference_index(ds, node_ids, decoded(ds.distance, ds.dimensions, values), roots)
    for off in (1, 2, 3):
        bufs = [np.zeros(len(v) + off, np.uint8) for v in values]
        for b, v in zip(bufs, values):
            b[off:] = np.frombuffer(v, np.uint8)
        views = [b[off:] for b in bufs]
        ix = Index.from_encoded(ds, node_ids, views, roots)
        assert_same_index(ix, ref)
        ix.close()
    ref.close()
    empty, stats = Index.from_encoded(ds, [], [], [], want_stats=True)
    ref = reference_index(ds, [], [], [])
    assert_same_index(empty, ref)
    assert stats["values"] == 0 and stats["chunks"] == 0 and empty.export_info()["n_nodes"] == 0
    empty.close(), ref.close(), ds.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good():
    ds, vecs = make(D.Euclidean, 600, 30, seed=6, duplicates=30)
    node_ids, values, roots = stream_values(ds, [5, 6, 7], split_after=20)
    yield ds, vecs, node_ids, values, roots
    ds.close()


TWO_KEYS = node_codec.encode_descendants(np.array([1, 5, 70000, 70001], np.uint32))  # pairs at 9, offsets at 17, bodies at 25


def run_value(runs, card, key=0):
    return desc_value([(key, roaring.RUN, card, roaring.run_body([s for s, _ in runs], [l for _, l in runs]))], True)


def unsorted_array():
    lows = np.arange(100) * 3
    lows[64] = lows[63]  # the first id of the second 64-id step of the wave against the last of the first
    return desc_value([(0, roaring.ARRAY, 100, roaring.array_body(lows))], False)


def descending_array():
    lows = np.arange(200) * 3
    lows[128] = lows[127] - 1
    return desc_value([(0, roaring.ARRAY, 200, roaring.array_body(lows)), (1, roaring.RUN, 3, roaring.run_body([4], [2]))], True)


def crowded_bitmap():
    return desc_value([(0, roaring.BITMAP, 5000, roaring.bitmap_body(np.arange(5001) * 2))], False)


VALUE_CASES = {  # name -> (which kind of value is replaced, its replacement as a function of the good value, the reason's words)
    "tag_0": ("leaf", lambda v: b"\0" + v[1:], "unknown node tag"),
    "tag_7": ("split", lambda v: b"\7" + v[1:], "unknown node tag"),
    "split_length_10": ("none_split", lambda v: v + b"\0", "split value"),
    "split_one_short": ("split", lambda v: v[:-1], "split value"),
    "child_absent": ("split", lambda v: v[:1] + struct.pack(">I", 5) + v[5:], "child id"),
    "cookie_12345": ("leaf", lambda v: TWO_KEYS[:1] + struct.pack("<I", 12345) + TWO_KEYS[5:], "cookie"),
    "keys_descending": ("leaf", lambda v: TWO_KEYS[:9] + TWO_KEYS[13:17] + TWO_KEYS[9:13] + TWO_KEYS[17:], "keys"),
    "container_past_the_end": ("leaf", lambda v: TWO_KEYS[:-1], "past the end"),
    "wrong_offset_entry": ("leaf", lambda v: TWO_KEYS[:21] + struct.pack("<I", 30) + TWO_KEYS[25:], "offset entry"),
    "trailing_byte": ("leaf", lambda v: TWO_KEYS + b"\0", "behind the last container"),
    "array_equal_across_lanes": ("leaf", lambda v: unsorted_array(), "array container"),
    "array_descending_on_a_block": ("leaf", lambda v: descending_array(), "array container"),
    "bitmap_one_bit_too_many": ("leaf", lambda v: crowded_bitmap(), "popcount"),
    "runs_overlap": ("leaf", lambda v: run_value([(0, 10), (5, 3)], 15), "overlap"),
    "run_past_65535": ("leaf", lambda v: run_value([(65530, 10)], 11), "past 65535"),
    "run_cardinality_off_by_one": ("leaf", lambda v: run_value([(0, 9)], 11), "total length"),
}


def refused(ds, node_ids, values, roots):
    with pytest.raises(_lib.ArroyHipError) as e:
        Index.from_encoded(ds, node_ids, values, roots)
    assert e.value.status == INVALID_ARGUMENT, str(e.value)
    return str(e.value)


def test_malformed_values_are_refused_by_name(good):
    ds, vecs, node_ids, values, roots = good
    bystander = Index.from_encoded(ds, node_ids, values, roots)  # (another index of the dataset stays searchable meanwhile)
    before = bystander.search(5, queries=vecs[:4], search_k=100)
    Index.from_encoded(ds, node_ids, values, roots).close()
    filters_before, live_before = bystander.filter_stats(), _lib.device_cache_stats(0)[0]
    leaves = [i for i, v in enumerate(values) if v[0] == 1]
    splits = [i for i, v in enumerate(values) if v[0] == 2 and len(v) > 9]
    none_splits = [i for i, v in enumerate(values) if len(v) == 9]
    assert leaves and splits and none_splits
    behind = [i for i in splits if i > min(leaves)]  # (a leaf in front of it can be made the smaller bad position)
    pick = {"leaf": leaves[len(leaves) // 3], "split": behind[len(behind) // 3], "none_split": none_splits[0]}
    assert min(leaves) < pick["leaf"] and pick["split"] < max(leaves)
    for name, (kind, mutate, words) in VALUE_CASES.items():
        at = pick[kind]
        bad = list(values)
        bad[at] = mutate(values[at])
        msg = refused(ds, node_ids, bad, roots)
        assert f"node {node_ids[at]} " in msg and words in msg, (name, msg)
        # two bad values: the smaller position is named, whichever pass finds which
        later = max(i for i in leaves if i > at)
        bad[later] = b"\7" + bad[later][1:]
        msg = refused(ds, node_ids, bad, roots)
        assert f"node {node_ids[at]} " in msg and words in msg, (name, "with a bad tag behind it", msg)
        earlier = min(leaves)
        if earlier < at:
            bad[earlier] = unsorted_array()
            msg = refused(ds, node_ids, bad, roots)
            assert f"node {node_ids[earlier]} " in msg and "array container" in msg, (name, "with a bad array in front of it", msg)
    # structure
    msg = refused(ds, node_ids, values, roots[:-1] + [5])
    assert "root 2 (node 5)" in msg and "root id" in msg, msg
    swapped = list(node_ids)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    assert "ascending at position 4" in refused(ds, swapped, values, roots)
    a, b = splits[0], splits[-1]
    two_parents = list(values)
    two_parents[b] = values[b][:1] + values[a][1:5] + values[b][5:]  # b's left child is a's
    msg = refused(ds, node_ids, two_parents, roots)
    assert "reachable twice" in msg and "node %d " % struct.unpack(">I", values[a][1:5])[0] in msg, msg
    for args in ((None, values, roots), (node_ids, None, roots), (node_ids, values, None)):
        n = len(node_ids)
        ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(v), C.c_void_p).value for v in values])
        lens = (C.c_size_t * n)(*[len(v) for v in values])
        ids, rts, h = np.array(node_ids, np.uint32), np.array(roots, np.uint32), C.c_void_p(99)
        st = _lib.lib().ah_index_create_from_encoded(ds._h, None if args[0] is None else ids.ctypes.data, None if args[1] is None else ptrs,
                                                     lens, n, None if args[2] is None else rts.ctypes.data, len(roots), C.byref(h), None)
        assert st == INVALID_ARGUMENT and b"NULL" in _lib.lib().ah_last_error() and h.value is None
    pending = Dataset(D.Euclidean, 30, 10)  # not finalized
    with pytest.raises(_lib.ArroyHipError) as e:
        Index.from_encoded(pending, node_ids, values, roots)
    assert e.value.status == 7
    pending.close()
    # nothing is held: no filter, no block, and the dataset is free again once its indexes are gone
    assert bystander.filter_stats() == filters_before and _lib.device_cache_stats(0)[0] == live_before
    assert bystander.search(5, queries=vecs[:4], search_k=100) == before
    bystander.close()
    ds.update_vectors([], [599], vecs[599:600])


def test_every_allocation_of_the_call_may_fail(good):
    ds, _vecs, node_ids, values, roots = good
    ref = reference_index(ds, node_ids, decoded(ds.distance, ds.dimensions, values), roots)
    largest = max((len(v) + 15) & ~15 for v in values)
    with _lib.tuning(AH_DECODE_CHUNK_BYTES=40 * largest):  # a few chunks: the arrays grow between them
        seen = sweep(lambda: Index.from_encoded(ds, node_ids, values, roots), cleanup=lambda ix: ix.close())
        assert len(seen) >= 8 and OOM in seen and all(s in (OOM, DEVICE) for s in seen), seen
        ix = Index.from_encoded(ds, node_ids, values, roots)
    assert_same_index(ix, ref)
    ix.close(), ref.close()


def test_maintenance_of_an_opened_index(good):
    ds, _vecs, node_ids, values, roots = good
    ix, ref, _stats = check(ds, node_ids, values, roots)
    gone = np.arange(3, 600, 5, dtype=np.uint32)
    da, db = ix.delete_items(gone, 20), ref.delete_items(gone, 20)
    assert da.keys() == db.keys() and all(da[k].tobytes() == db[k].tobytes() for k in da)
    assert_same_index(ix, ref)
    assert ix.compact() == ref.compact()
    assert_same_index(ix, ref)
    assert ix.audit()["bad_link"] == 0 and ix.footprint()["free_slots"] == 0
    ix.close(), ref.close()
