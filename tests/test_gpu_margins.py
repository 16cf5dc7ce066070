"""`ah_margins` — `D::margin(&normal, query_leaf)` for many stored normals (src/reader.rs:366-369) — against the oracle, bit for bit.

It is the only caller of `launch_split_sides(..., row_is_normal = 1)`: the branch of `k_split_sides_f32<M>` and
`k_split_sides_bq` in which the rows are the normals, the bias comes from the ROW's header and DotProduct's `extra_dim` product is
taken between the leaf's header and the row's.  The reference is the oracle's margin of a stored item against a normal,
`Data.split_sides(nv_i, nh_i, rows=[leaf_row])`, with the leaves as the rows of a small oracle `Data`.  The last two sections run
both single-node kernels past one grid (2048 blocks) through `ah_margins` and through `ah_split_sides`, and descend whole trees
on the host by the sign of the margins."""
import ctypes as C

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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.nonzero(bits(a) != bits(b))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a[bad[:5]]} vs {b[bad[:5]]}"


ALL_METRICS = [0, 1, 2, 3, 4, 5, 6]
DIMS = [3, 17, 30, 32, 70, 100, 768]  # f32: scalar, SSE and AVX tiers; 1-bit: one, two and twelve words
N_NORMALS = 300


# ---- the two sides ------------------------------------------------------------------------------------------------------

def items_of(metric, dims, n, seed):
    """Random stored items in the oracle (DotProduct preprocessed: real, non-zero extra_dims)."""
    vecs = np.random.default_rng(seed).standard_normal((n, dims)).astype(np.float32)
    data = O.Data(metric, vecs)
    if metric == 3:
        data.preprocess_dot()
    return data, vecs


def normals_from_splits(data, n_normals, seed):
    """(vectors [n, vector_bytes] u8, headers [n, header_floats] f32) of `create_split` over random samples of `data`."""
    rng = np.random.default_rng(seed)
    nvs, nhs = [], []
    for _ in range(n_normals):
        sample = rng.choice(data.n, 12, replace=False).astype(np.uint32)
        nv, nh = data.create_split(sample)
        nvs.append(nv)
        nhs.append(nh)
    return np.stack(nvs), np.stack(nhs).astype(np.float32)


def stage_normals(metric, dims, nvs, nhs, ids=None):
    """The normals as the ITEMS of a dataset: records `[0u8][header][codec bytes]`, one contiguous host buffer."""
    from arroy_amd import Dataset
    cls = D.BY_METRIC[metric]
    n = len(nvs)
    hs, vs = cls.header_size(), cls.vector_size(dims)
    assert nvs.shape == (n, vs) and nhs.shape == (n, hs // 4)
    rec = np.zeros((n, 1 + hs + vs), dtype=np.uint8)
    rec[:, 1:1 + hs] = np.ascontiguousarray(nhs, dtype="<f4").view(np.uint8).reshape(n, hs)
    rec[:, 1 + hs:] = nvs
    ids = np.arange(n, dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
    ds = Dataset(cls, dims, n)
    if n <= 4096:
        ds.upload_records(ids, [r.tobytes() for r in rec], preprocessed=True)
    else:  # the same call from one buffer (the wrapper above copies every record into its own ctypes buffer)
        assert metric != 3
        ds.upload_record_pointers(ids, rec.ctypes.data + np.arange(n, dtype=np.int64) * rec.shape[1], rec.shape[1])
    ds.finalize()
    return ds


def leaf_data(metric, dims, leaves):
    """The leaves `(codec bytes, header f32[2])` as the rows of an oracle Data, headers as given."""
    hf = O.header_floats(metric)
    codec = np.stack([np.ascontiguousarray(v).view(np.uint8).ravel() for v, _ in leaves])
    hdrs = np.stack([np.asarray(h, dtype=np.float32)[:hf] for _, h in leaves])
    vecs = codec.view(np.float32).reshape(len(leaves), dims) if not O.is_bq(metric) else np.zeros((len(leaves), dims), np.float32)
    return O.Data(metric, vecs, headers=hdrs, codec_bytes=codec)


def oracle_margins(metric, dims, nvs, nhs, leaves):
    """[n_leaves, n_normals]: for normal i, `split_sides(nv_i, nh_i, rows=[leaf])` of the oracle, the margins only."""
    ld = leaf_data(metric, dims, leaves)
    L = O.lib()
    n, k = len(nvs), len(leaves)
    out = np.zeros((n, k), dtype=np.float32)
    rows = np.arange(k, dtype=np.uint32)
    sides = np.zeros(k, dtype=np.uint8)
    nl = C.c_uint64(0)
    nv = np.ascontiguousarray(nvs)
    nh = np.zeros((n, 2), dtype=np.float32)
    nh[:, : nhs.shape[1]] = nhs
    vstep, base_v, base_h, base_o = nv.shape[1], nv.ctypes.data, nh.ctypes.data, out.ctypes.data
    cdata, prow, psides, pnl = ld.c(), rows.ctypes.data, sides.ctypes.data, C.byref(nl)
    for i in range(n):
        L.ao_split_sides(cdata, base_v + i * vstep, base_h + i * 8, prow, k, psides, pnl, base_o + i * 4 * k)
    return out.T.copy()


# ---- parity: every metric, every tier, both kinds of leaf ---------------------------------------------------------------

@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("dims", DIMS)
def test_margins_equal_the_oracle_for_query_and_item_leaves(metric, dims):
    data, vecs = items_of(metric, dims, 400, seed=1000 + 37 * metric + dims)
    nvs, nhs = normals_from_splits(data, N_NORMALS, seed=dims + metric)
    hf = O.header_floats(metric)
    if metric in (0, 1, 4, 5):
        assert np.count_nonzero(nhs[:, 0]) > N_NORMALS // 2, "the biases of the staged normals must be real"
    ds = stage_normals(metric, dims, nvs, nhs)
    assert len(ds) == N_NORMALS
    q = np.random.default_rng(dims).standard_normal(dims).astype(np.float32)
    leaves = [data.query_leaf(q), data.item_leaf(7), data.item_leaf(123)]  # by_vector (new_header), by_item x 2
    if metric == 3:
        assert leaves[0][1][0] == 0.0 and leaves[1][1][0] != 0.0, "the by_item DotProduct leaf is the one with an extra_dim"
    want = oracle_margins(metric, dims, nvs, nhs, leaves)
    for j, (lv, lh) in enumerate(leaves):
        assert_bit_equal(ds.margins(lv, lh[:hf]), want[j], f"m={metric} d={dims} leaf {j}")
    ds.close()


# ---- which header is read ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 1, 4, 5])
@pytest.mark.parametrize("dims", [30, 100])
def test_the_bias_is_the_rows_not_the_leafs(metric, dims):
    data, vecs = items_of(metric, dims, 200, seed=5 + metric)
    nvs, nhs = normals_from_splits(data, 100, seed=dims)
    ds = stage_normals(metric, dims, nvs, nhs)
    lv, lh = data.item_leaf(11)
    want = oracle_margins(metric, dims, nvs, nhs, [(lv, lh)])[0]
    for first in (lh[0], 1.0e6, -3.5e4):  # the leaf's own header is no operand of D::margin for these metrics
        assert_bit_equal(ds.margins(lv, [first]), want, f"leaf header {first}")
    assert np.count_nonzero(nhs[:, 0]) > 50, "the biases of the staged normals must be real"
    ds.close()


@pytest.mark.parametrize("dims", [17, 100])
def test_dot_product_multiplies_the_leafs_extra_dim_with_the_rows(dims):
    data, vecs = items_of(3, dims, 200, seed=8)
    nvs, nhs = normals_from_splits(data, 100, seed=dims)
    assert np.count_nonzero(nhs[:, 0]) > 50, "the normals' extra_dims must be real"
    ds = stage_normals(3, dims, nvs, nhs)
    lv, lh = data.item_leaf(5)
    a, b = np.array([0.0, lh[1]], np.float32), np.array([lh[0] + np.float32(1.5), lh[1]], np.float32)
    want = oracle_margins(3, dims, nvs, nhs, [(lv, a), (lv, b), (lv, lh)])
    got = [ds.margins(lv, h) for h in (a, b, lh)]
    for j in range(3):
        assert_bit_equal(got[j], want[j], f"leaf header {j}")
    assert np.count_nonzero(bits(got[0]) != bits(got[1])) > 50, "two leaves that differ in extra_dim must differ in margins"
    # the norm of either header is no operand
    assert_bit_equal(ds.margins(lv, [lh[0], 99.0]), want[2])
    ds.close()


# ---- gather and id handling --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 3, 6])
@pytest.mark.parametrize("id_kind", ["dense", "sparse_lut", "sparse_search"])
def test_margins_of_listed_ids(metric, id_kind):
    from arroy_amd import MissingKey
    dims, n = 40, 200
    data, vecs = items_of(metric, dims, 300, seed=21 + metric)
    nvs, nhs = normals_from_splits(data, n, seed=3)
    rng = np.random.default_rng(4)
    ids = {"dense": np.arange(n, dtype=np.uint32),
           "sparse_lut": np.sort(rng.choice(5000, n, replace=False)).astype(np.uint32),
           "sparse_search": (np.arange(n, dtype=np.uint64) * 20_000_000 + 7).astype(np.uint32)}[id_kind]
    ds = stage_normals(metric, dims, nvs, nhs, ids=ids)
    hf = O.header_floats(metric)
    lv, lh = data.item_leaf(9)
    want = oracle_margins(metric, dims, nvs, nhs, [(lv, lh)])[0]
    assert_bit_equal(ds.margins(lv, lh[:hf]), want, "every normal in row order")
    unsorted = rng.permutation(n)[:77]
    for what, rows in (("strided", np.arange(1, n, 3)), ("unsorted", unsorted), ("repeated", np.array([5, 5, 0, 199, 5, 0, 198])),
                       ("one", np.array([n - 1]))):
        assert_bit_equal(ds.margins(lv, lh[:hf], item_ids=ids[rows]), want[rows], what)
    missing = int(ids[-1]) + 1 if id_kind != "sparse_lut" else int(np.setdiff1d(np.arange(5000), ids)[3])
    with pytest.raises(MissingKey):
        ds.margins(lv, lh[:hf], item_ids=np.concatenate([ids[:40], [missing], ids[40:50]]))
    assert_bit_equal(ds.margins(lv, lh[:hf], item_ids=ids[:3]), want[:3], "usable after the refusal")
    ds.close()


def test_edge_calls():
    from arroy_amd import ArroyHipError, Dataset, _lib
    dims = 32
    data, vecs = items_of(0, dims, 50, seed=2)
    nvs, nhs = normals_from_splits(data, 20, seed=1)
    ds = stage_normals(0, dims, nvs, nhs)
    lv, lh = data.item_leaf(0)
    got = ds.margins(lv, lh[:1], item_ids=np.zeros(0, np.uint32))
    assert got.shape == (0,)
    out = np.full(4, 7.0, np.float32)
    ids = np.zeros(4, np.uint32)
    L = _lib.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lvb, lhb = np.ascontiguousarray(lv), np.zeros(2, np.float32)
    assert L.ah_margins(ds._h, vp(lvb), vp(lhb), vp(ids), 0, vp(out)) == 0 and np.all(out == 7.0), "n == 0 with ids: nothing written"
    assert L.ah_margins(ds._h, None, vp(lhb), vp(ids), 4, vp(out)) == 5, "a NULL leaf vector is an invalid argument"
    assert L.ah_margins(ds._h, vp(lvb), None, vp(ids), 4, vp(out)) == 5, "a NULL leaf header is an invalid argument"
    assert L.ah_margins(ds._h, vp(lvb), vp(lhb), None, 0, None) == 5, "NULL ids mean every normal: a NULL output is refused"
    assert L.ah_margins(None, vp(lvb), vp(lhb), None, 0, vp(out)) == 5
    assert np.all(out == 7.0)
    fresh = Dataset(D.Euclidean, dims, 4)
    fresh.upload_vectors(np.arange(4), vecs[:4])
    with pytest.raises(ArroyHipError) as e:
        fresh.margins(lv, lh[:1])
    assert e.value.status == 7, "an unfinalized dataset is refused"
    fresh.close()
    ds.close()


# ---- past one grid: 2048 blocks x 32 octets (f32), 2048 x 256 threads (1-bit) ---------------------------------------------

F32_PAST_GRID = (65_536 + 33, 32)
BQ_PAST_GRID = (524_288 + 65, 64)


@pytest.fixture(scope="module")
def f32_rows():
    n, dims = F32_PAST_GRID
    rng = np.random.default_rng(77)
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    bias = rng.standard_normal((n, 1)).astype(np.float32)
    q = rng.standard_normal(dims).astype(np.float32)
    return vecs, bias, q


@pytest.fixture(scope="module")
def bq_rows():
    n, dims = BQ_PAST_GRID
    rng = np.random.default_rng(78)
    words = rng.integers(0, 2**64, size=(n, 1), dtype=np.uint64)
    bias = rng.integers(-40, 41, size=(n, 1)).astype(np.float32) + np.float32(0.5)
    q = rng.integers(0, 2**64, size=1, dtype=np.uint64)
    return words, bias, q


def test_margins_past_one_grid_f32(f32_rows):
    vecs, bias, q = f32_rows
    n, dims = F32_PAST_GRID
    assert n > 2048 * 32
    ds = stage_normals(0, dims, vecs.view(np.uint8).reshape(n, 4 * dims), bias)
    lh = np.array([123.0], np.float32)
    want = oracle_margins(0, dims, vecs.view(np.uint8).reshape(n, 4 * dims), bias, [(q, lh)])[0]
    assert_bit_equal(ds.margins(q, lh), want, "every row")
    rows = np.array([0, 65_535, 65_536, n - 1, 2048 * 32 - 1, 40_000, 65_540], dtype=np.uint32)
    assert_bit_equal(ds.margins(q, lh, item_ids=rows), want[rows], "rows of both sweeps, gathered")
    ds.close()


def bq_exact_margins(words, bias, q):
    """bias + (64 * words - 2 * hamming): the 1-bit dot product in integers, one exact f32 addition."""
    x = words ^ q[None, :]
    ham = np.unpackbits(x.view(np.uint8), axis=1).sum(axis=1).astype(np.int64)
    return (bias[:, 0] + (64 * words.shape[1] - 2 * ham).astype(np.float32)).astype(np.float32)


def test_margins_past_one_grid_1bit(bq_rows):
    words, bias, q = bq_rows
    n, dims = BQ_PAST_GRID
    assert n > 2048 * 256
    codec = words.view(np.uint8).reshape(n, 8)
    ds = stage_normals(4, dims, codec, bias)
    got = ds.margins(q.view(np.uint8), [55.0])
    assert_bit_equal(got, bq_exact_margins(words, bias, q), "every row, integer form")
    sample = np.unique(np.concatenate([np.arange(0, n, 1777), np.arange(n - 300, n)]))
    want = oracle_margins(4, dims, codec[sample], bias[sample], [(q.view(np.uint8), np.array([55.0], np.float32))])[0]
    assert_bit_equal(got[sample], want, "strided sample and the last 300 rows, oracle")
    ds.close()


# ---- the same two shapes through ah_split_sides: its kernels' second sweep -------------------------------------------------

def check_split_sides(ds, data, nv, nh, n):
    sides, n_left, margins = ds.split_sides(nv, nh)
    es, enl, em = data.split_sides(nv, nh)
    assert_bit_equal(margins, em, "margins")
    assert sides.shape == (n,) and np.array_equal(sides, es), "side bits, the last partial word included"
    assert n_left == enl == int(n - es.sum())
    assert 0 < n_left < n
    return sides


def test_split_sides_past_one_grid_f32(f32_rows):
    from arroy_amd import Dataset
    vecs, bias, q = f32_rows
    n, dims = F32_PAST_GRID
    assert n % 32 != 0
    ds = Dataset(D.Euclidean, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    ds.finalize()
    data = O.Data(0, vecs)
    check_split_sides(ds, data, q.view(np.uint8), np.array([0.25], np.float32), n)
    sub = np.arange(3, n, dtype=np.uint32)  # a gathered list that is still more than one grid
    sides, n_left, margins = ds.split_sides(q.view(np.uint8), [0.25], sorted_ids=sub)
    es, enl, em = data.split_sides(q.view(np.uint8), np.array([0.25], np.float32), rows=sub)
    assert_bit_equal(margins, em)
    assert np.array_equal(sides, es) and n_left == enl
    ds.close()


def test_split_sides_past_one_grid_1bit(bq_rows):
    from arroy_amd import Dataset
    words, bias, q = bq_rows
    n, dims = BQ_PAST_GRID
    assert n % 32 != 0
    codec = words.view(np.uint8).reshape(n, 8)
    rec = np.zeros((n, 13), dtype=np.uint8)
    rec[:, 5:] = codec
    ds = Dataset(D.BinaryQuantizedEuclidean, dims, n)
    ds.upload_record_pointers(np.arange(n, dtype=np.uint32), rec.ctypes.data + np.arange(n, dtype=np.int64) * 13, 13)
    ds.finalize()
    data = O.Data(4, np.zeros((n, dims), np.float32), headers=np.zeros((n, 1), np.float32), codec_bytes=codec)
    check_split_sides(ds, data, q.view(np.uint8), np.array([-1.0], np.float32), n)
    ds.close()


# ---- a host-side descent by the sign of the margins -----------------------------------------------------------------------

@pytest.mark.parametrize("metric,dims", [(0, 48), (6, 256)])
def test_host_descent_by_margins_reaches_the_routed_leaf(metric, dims):
    from arroy_amd import Dataset
    cls = D.BY_METRIC[metric]
    n, seeds = 2000, [11, 12, 13]
    vecs = np.random.default_rng(90 + metric).standard_normal((n, dims)).astype(np.float32)
    ds = Dataset(cls, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    ds.finalize()
    data = O.Data(metric, vecs)
    forest = ds.build_forest(seeds, split_after=16)
    index = ds.create_index(forest)
    nodes = forest.nodes
    planes = [i for i in range(len(nodes)) if nodes[i]["kind"] == 2 and nodes[i]["has_normal"]]
    normals = [forest.normal_of(i) for i in planes]
    nds = stage_normals(metric, dims, np.stack([v for _, v in normals]), np.stack([h for h, _ in normals]),
                        ids=np.array(planes, dtype=np.uint32))  # item id = the split node's index in the view
    row_of = {node: r for r, node in enumerate(planes)}
    items = np.random.default_rng(1).choice(n, 40, replace=False).astype(np.uint32)
    routed = index.route_items(items, seeds)
    assert np.array_equal(routed, O.route_items(data, forest, items, seeds))
    hf = O.header_floats(metric)
    left_out = walked = 0
    for k, item in enumerate(items):
        lv, lh = data.item_leaf(int(item))
        m = nds.margins(lv, lh[:hf])
        for t in range(len(seeds)):
            node = int(forest.roots[t])
            while nodes[node]["kind"] == 2 and node in row_of:
                right = (bits(m[row_of[node]])[()] >> 31) == 0  # D::side: Right iff the sign bit is clear
                node = int(nodes[node]["right" if right else "left"])
            if nodes[node]["kind"] == 2:  # a split without a normal: the routing flips a coin the margins know nothing of
                left_out += 1
                continue
            walked += 1
            assert node == int(routed[t, k]), f"item {item} tree {t}: the margins lead to node {node}, the routing to {routed[t, k]}"
            assert int(item) in forest.descendants_of(node)
    print(f"host descent m={metric}: {walked} paths walked, {left_out} left out (a split without a normal)")
    assert left_out * 20 <= len(items) * len(seeds), f"{left_out} of {len(items) * len(seeds)} paths left out"
    for handle in (nds, index, forest, ds):
        handle.close()
