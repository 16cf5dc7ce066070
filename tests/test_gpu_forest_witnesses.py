"""The witnesses of the forest tests are themselves checked: `ah_forest_digest`, `ah_forest_digest_keyed`, `ah_forest_visit`.

`Forest.digest()[0] == ...` is the only assertion of some 35 GPU tests and the correctness gate of bench.py; a digest that
skipped a field would blind all of them at once.  Here the digest is restated in plain Python from its contract in
include/arroy_hip.h (per tree, in view order: kind / has_normal / depth / count of every node, the children relative to the tree's
first node, vector and header bytes of every split plane, the ids of every Descendants node, the tree's key), must equal the
library's value exactly, and is shown to move with every one of those fields — which pins the C digest to each of them."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = None
O = None


@pytest.fixture(scope="module", autouse=True)
def _imports():
    global D, O
    import arroy_amd
    from arroy_amd import distances
    from oracle import oracle
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    D, O = distances, oracle


# ---- the digest, restated ------------------------------------------------------------------------------------------------

M64 = (1 << 64) - 1


def mix64(x):
    """ah_mix64 (include/arroy_hip_policy.h): the splitmix64 finaliser."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def rotl64(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


LANE_MUL = (0x9FB21C651E98DF25, 0xD6E8FEB86659FD93, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB)
LANE_ROT = (29, 31, 27, 33)


def hash_bytes(data: bytes, seed: int) -> int:
    """`hash_bytes` (forest.hip): four multiply-rotate lanes over 32-byte blocks of little-endian u64 words; the last, partial
    block zero-padded and multiplied without the rotation (always, also when it is empty); the lanes folded with mix64 and the
    length."""
    n = len(data)
    h = [seed ^ 0x9E3779B97F4A7C15, (seed + 0xC2B2AE3D27D4EB4F) & M64, ~seed & M64, (seed * 0x165667B19E3779F9 + n) & M64]
    full = n - n % 32
    for i in range(0, full, 32):
        w = struct.unpack_from("<4Q", data, i)
        h = [rotl64(((h[k] ^ w[k]) * LANE_MUL[k]) & M64, LANE_ROT[k]) for k in range(4)]
    w = struct.unpack("<4Q", data[full:] + bytes(32 - (n - full)))
    h = [((h[k] ^ w[k]) * LANE_MUL[k]) & M64 for k in range(4)]
    return mix64((mix64(h[0] ^ rotl64(h[1], 17)) + mix64(h[2] ^ rotl64(h[3], 41)) + n) & M64)


class View:
    """Copies of the arrays of an ah_forest_view (the tests below change them)."""

    def __init__(self, forest):
        self.n_trees = forest.n_trees
        self.nodes = forest.nodes.copy()
        self.normals = forest.normals.copy()
        self.descendants = forest.descendants.copy()
        self.stride, self.vec_off, self.hdr_off = forest.normal_stride, forest._vec_off, forest._hdr_off


def restated_digest(v: View, keys=None):
    """(total, per tree) by the recipe of include/arroy_hip.h."""
    per = []
    tree_of = v.nodes["tree"]
    for t in range(v.n_trees):
        mine = np.nonzero(tree_of == t)[0]
        base = int(mine[0]) if mine.size else 0
        h = mix64((0x61727279 + (t if keys is None else int(keys[t]))) & M64)
        for i in mine:
            nd = v.nodes[i]
            split = int(nd["kind"]) == 2
            fields = (int(nd["kind"]) | int(nd["has_normal"]) << 8 | int(nd["depth"]) << 32, int(nd["count"]),
                      (int(nd["left"]) - base) & M64 if split else 0, (int(nd["right"]) - base) & M64 if split else 0)
            h = mix64(h ^ hash_bytes(struct.pack("<4Q", *fields), int(i) - base))
            off = int(nd["offset"])
            if split:
                if nd["has_normal"]:
                    rec = v.normals[off: off + v.stride].tobytes()
                    h = mix64(h ^ hash_bytes(rec[v.vec_off: v.hdr_off], 1))
                    h = mix64(h ^ hash_bytes(rec[v.hdr_off: v.hdr_off + 8], 2))
            else:
                h = mix64(h ^ hash_bytes(v.descendants[off: off + int(nd["count"])].astype("<u4").tobytes(), 3))
        per.append(h)
    total = mix64(v.n_trees)
    for h in per:
        total = mix64(total ^ h)
    return total, per


# ---- forests -------------------------------------------------------------------------------------------------------------

N_ROWS, SEEDS, SPLIT_AFTER = 2000, [101, 202, 303, 404], 24


def staged(metric, dims, vecs):
    from arroy_amd import Dataset
    ds = Dataset(D.BY_METRIC[metric], dims, len(vecs))
    ds.upload_vectors(np.arange(len(vecs), dtype=np.uint32), vecs)
    if metric == 3:
        ds.preprocess_dot()
    return ds.finalize()


def random_rows(dims, seed=5, n=N_ROWS):
    return np.random.default_rng(seed).standard_normal((n, dims)).astype(np.float32)


FORESTS = {
    "euclidean": dict(metric=0, dims=40),
    "dot_product": dict(metric=3, dims=33),
    "bq_cosine": dict(metric=6, dims=200),
    "identical_rows": dict(metric=0, dims=32, identical=True, split_after=8),
    "two_batches": dict(metric=2, dims=64, max_trees_in_flight=2),
}


@pytest.fixture(scope="module")
def forests():
    made = {}

    def get(name):
        if name not in made:
            spec = {"split_after": SPLIT_AFTER, **FORESTS[name]}
            metric, dims = spec.pop("metric"), spec.pop("dims")
            vecs = random_rows(dims)
            if spec.pop("identical", False):
                vecs[:] = vecs[0]
            ds = staged(metric, dims, vecs)
            made[name] = (ds, ds.build_forest(SEEDS, **spec))
        return made[name]
    yield get
    for ds, forest in made.values():
        forest.close()
        ds.close()


@pytest.mark.parametrize("name", list(FORESTS))
def test_the_digest_is_the_restated_one(forests, name):
    ds, forest = forests(name)
    total, per = forest.digest()
    want_total, want_per = restated_digest(View(forest))
    assert [int(x) for x in per] == want_per, "per-tree digests"
    assert total == want_total
    nodes = forest.nodes
    assert forest.n_trees == 4 and len(nodes) > 100
    no_normal = int(np.count_nonzero((nodes["kind"] == 2) & (nodes["has_normal"] == 0)))
    if name == "identical_rows":
        assert no_normal > 0, "identical rows are split by the random fallback"
    if name == "two_batches":
        one = ds.build_forest(SEEDS, split_after=SPLIT_AFTER)
        assert one.digest()[0] == total, "the batching is no content"
        one.close()
    assert len(set(want_per)) == 4


def a_node(v, pred):
    for i in range(len(v.nodes) // 3, len(v.nodes)):  # (not the first node of a tree)
        if pred(v.nodes[i]):
            return i
    raise AssertionError("no such node")


@pytest.mark.parametrize("name", ["euclidean", "dot_product", "bq_cosine"])
def test_the_restatement_moves_with_every_field(forests, name):
    """With the equality above: the C digest reads every field the header says it reads."""
    ds, forest = forests(name)
    base_total, base_per = restated_digest(View(forest))
    cls = forest.distance
    hs, vs = cls.header_size(), cls.vector_size(forest.dimensions)

    def changed(what, change):
        v = View(forest)
        tree = change(v)
        total, per = restated_digest(v)
        assert total != base_total, what
        assert [a != b for a, b in zip(per, base_per)] == [t == tree for t in range(4)], f"{what}: only tree {tree} changes"

    def is_split(nd):
        return nd["kind"] == 2 and nd["has_normal"]

    def one_id(v):
        i = a_node(v, lambda nd: nd["kind"] == 1 and nd["count"] > 1)
        v.descendants[int(v.nodes[i]["offset"]) + int(v.nodes[i]["count"]) - 1] ^= 1
        return int(v.nodes[i]["tree"])

    def vector_byte(at):
        def change(v):
            i = a_node(v, is_split)
            v.normals[int(v.nodes[i]["offset"]) + v.vec_off + at] ^= 0x10
            return int(v.nodes[i]["tree"])
        return change

    def header_byte(at):
        def change(v):
            i = a_node(v, is_split)
            v.normals[int(v.nodes[i]["offset"]) + v.hdr_off + at] ^= 0x10
            return int(v.nodes[i]["tree"])
        return change

    def field(name_, kind, delta):
        def change(v):
            i = a_node(v, lambda nd: nd["kind"] == kind)
            v.nodes[name_][i] = int(v.nodes[name_][i]) + delta
            return int(v.nodes[i]["tree"])
        return change

    def kind_of_one(v):
        i = a_node(v, lambda nd: nd["kind"] == 1)
        tree = int(v.nodes[i]["tree"])
        v.nodes["kind"][i] = 2  # a split without a normal, its children the tree's first node: relative children 0, 0 as before
        v.nodes["left"][i] = v.nodes["right"][i] = int(np.nonzero(v.nodes["tree"] == tree)[0][0])
        return tree

    changed("one id", one_id)
    changed("first vector byte", vector_byte(0))
    changed("last vector byte", vector_byte(vs - 1))
    changed("first header byte", header_byte(0))
    changed("last header byte", header_byte(hs - 1))
    changed("left child", field("left", 2, -1))
    changed("right child", field("right", 2, -1))
    changed("count of a split", field("count", 2, 1))
    changed("depth of a split", field("depth", 2, 1))
    changed("depth of a Descendants node", field("depth", 1, 1))
    changed("has_normal", field("has_normal", 1, 1))
    changed("kind", kind_of_one)
    # and what is NOT content: where a record or an id list lies, the padding rule aside
    v = View(forest)
    i = a_node(v, is_split)
    rec = v.normals[int(v.nodes[i]["offset"]): int(v.nodes[i]["offset"]) + v.stride].copy()
    v.normals = np.concatenate([v.normals, rec])
    v.nodes["offset"][i] = len(v.normals) - v.stride
    assert restated_digest(v) == (base_total, base_per), "the offset of a record is layout"


# ---- digest_keyed ------------------------------------------------------------------------------------------------------------

def test_digest_keyed(forests):
    ds, forest = forests("euclidean")
    total, per = forest.digest()
    assert np.array_equal(forest.digest_keyed(range(4)), per)
    even, odd = ds.build_forest(SEEDS[0::2], split_after=SPLIT_AFTER), ds.build_forest(SEEDS[1::2], split_after=SPLIT_AFTER)
    assert np.array_equal(even.digest_keyed([0, 2]), per[0::2]), "a share keyed by its trees' indices in the whole forest"
    assert np.array_equal(odd.digest_keyed([1, 3]), per[1::2])
    plain = even.digest()[1]
    assert int(plain[0]) == int(per[0]) and int(plain[1]) != int(per[2]), "unkeyed, tree 1 of the share is not tree 2 of the forest"
    keys = [7, 2**40 + 3, 2, 2**64 - 1]
    keyed = forest.digest_keyed(keys)
    assert [int(x) for x in keyed] == restated_digest(View(forest), keys)[1]
    for t in range(4):
        assert (int(keyed[t]) == int(per[t])) == (keys[t] == t), "a different key changes the value, the same one does not"
    from arroy_amd import _lib
    out = np.zeros(4, np.uint64)
    assert _lib.lib().ah_forest_digest_keyed(forest._h, None, out.ctypes.data_as(C.c_void_p)) == 5, "NULL keys are refused"
    even.close()
    odd.close()


# ---- digests against canonical() -------------------------------------------------------------------------------------------

def test_per_tree_digests_are_equal_exactly_where_the_trees_are(forests):
    dims = 40
    vecs = random_rows(dims)
    ds, forest = forests("euclidean")
    canon = [forest.canonical(t) for t in range(4)]
    per = forest.digest()[1]
    other_seed = list(SEEDS)
    other_seed[2] = 999
    moved = vecs.copy()
    moved[1234] += np.float32(0.75)
    moved_ds = staged(0, dims, moved)
    pairs = {"the same build twice": ds.build_forest(SEEDS, split_after=SPLIT_AFTER),
             "one seed changed": ds.build_forest(other_seed, split_after=SPLIT_AFTER),
             "split_after changed": ds.build_forest(SEEDS, split_after=SPLIT_AFTER - 4),
             "one row changed": moved_ds.build_forest(SEEDS, split_after=SPLIT_AFTER)}
    expect_equal = {"the same build twice": [True] * 4, "one seed changed": [True, True, False, True],
                    "split_after changed": [False] * 4}
    for what, other in pairs.items():
        same_tree = [other.canonical(t) == canon[t] for t in range(4)]
        same_digest = [int(a) == int(b) for a, b in zip(other.digest()[1], per)]
        assert same_digest == same_tree, what
        if what in expect_equal:
            assert same_tree == expect_equal[what], what
        else:
            assert not all(same_tree), what
        other.close()
    moved_ds.close()


# ---- ah_forest_visit ---------------------------------------------------------------------------------------------------------

SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t)


def visit(forest, stop_at=None):
    """ah_forest_visit with a Python sink -> (status, the calls); stop_at = k: the k-th call returns non-zero."""
    from arroy_amd import _lib
    calls = []

    def sink(_user, tree, node, kind, left, right, payload, payload_len):
        calls.append((tree, node, kind, left, right, None if not payload else C.string_at(payload, payload_len), payload_len))
        return 3 if stop_at is not None and len(calls) == stop_at else 0
    cb = SINK(sink)
    status = _lib.lib().ah_forest_visit(forest._h, C.cast(cb, C.c_void_p), None)
    return status, calls


@pytest.mark.parametrize("name", ["dot_product", "bq_cosine", "identical_rows", "two_batches"])
def test_visit_hands_every_node_to_the_sink(forests, name):
    from arroy_amd import _lib
    ds, forest = forests(name)
    status, calls = visit(forest)
    assert status == 0
    nodes = forest.nodes
    assert [c[1] for c in calls] == list(range(len(nodes))), "every node once, in view order"
    null_payloads = 0
    for tree, i, kind, left, right, payload, plen in calls:
        nd = nodes[i]
        assert (tree, kind) == (int(nd["tree"]), int(nd["kind"]))
        off = int(nd["offset"])
        if kind == 2:
            assert (left, right) == (int(nd["left"]), int(nd["right"]))
            assert left < i and right < i and int(nodes[left]["tree"]) == tree == int(nodes[right]["tree"]), "children before their parent"
            if nd["has_normal"]:
                assert plen == forest.normal_stride and payload == forest.normals[off: off + forest.normal_stride].tobytes()
            else:
                assert payload is None and plen == 0
                null_payloads += 1
        else:
            assert plen == 4 * int(nd["count"]) and payload == forest.descendants[off: off + int(nd["count"])].tobytes()
    assert null_payloads == int(np.count_nonzero((nodes["kind"] == 2) & (nodes["has_normal"] == 0)))
    assert null_payloads > 0 or name != "identical_rows"  # (coarse 1-bit margins leave some to the bq_cosine forest too)
    assert [int(forest.roots[t]) for t in range(4)] == [max(c[1] for c in calls if c[0] == t) for t in range(4)], "the root comes last"
    # a sink that stops the visit
    before = forest.digest()
    for k in (1, 17, len(nodes)):
        status, calls = visit(forest, stop_at=k)
        assert status == 2 and len(calls) == k, f"stopped at call {k}: status {status} after {len(calls)} calls"
        assert "stop" in _lib.lib().ah_last_error().decode()
    assert _lib.lib().ah_forest_visit(forest._h, None, None) == 5, "a NULL sink is refused"
    after = forest.digest()
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and visit(forest)[0] == 0, "usable afterwards"
