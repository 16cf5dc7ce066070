"""The f32 scan from the packed copy of the rows (AH_SCAN_PACKED): bit-equal to the scan of the f32 rows and to
the oracle, for the three metrics that use it, on plain and structured rows, rows built to be raw, rows with zeros and
denormals, at dims 32 / 96 / 640 / 768 / 1536 (last groups of 1, 3, 4 and 8 blocks), with the grid capped
(AH_SCAN_BLOCKS) so that the grid-stride loop runs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EUCLIDEAN, COSINE, DOT = 0, 2, 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rows(kind, n, dims, seed):
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return O.synth(seed, 1, n, dims)
    if kind == "normal":
        return rng.standard_normal((n, dims)).astype(np.float32)
    if kind == "clustered":
        return O.synth(seed, 4, n, dims)
    if kind == "low_rank":
        return O.synth(seed, 5, n, dims)
    assert kind == "edge"
    v = rng.uniform(-1, 1, (n, dims)).astype(np.float32)
    v[0::7, 3] *= np.float32(2.0 ** -14)   # spread 14..15: packed
    v[1::7, 5] *= np.float32(2.0 ** -16)   # spread 16..17: raw
    v[2::7, :dims // 2] = 0.0              # zeros: packed, code 15
    v[3::7, 1] = np.float32(-0.0)
    v[4::7, 2] = np.float32(1e-40)         # a denormal
    v[5::7] = np.float32(3.0)              # a constant row
    v[6::7] *= np.float32(2.0 ** 100)      # huge values
    return v


def scan_both(metric, vecs, q):
    """(packed scan, f32 scan, oracle, packed info) for one dataset."""
    from arroy_amd import Dataset, _lib, distances
    from oracle import oracle as O
    n, dims = vecs.shape
    ds = Dataset(distances.BY_METRIC[metric], dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    od = O.Data(metric, vecs)
    if metric == DOT:
        ds.preprocess_dot()
        od.preprocess_dot()
    ds.finalize()
    qv, qh = od.query_leaf(q)
    want = od.distances(qv, qh)
    with _lib.tuning(AH_SCAN_BLOCKS=8):  # 8 blocks of 32 octets: the grid-stride loop for n > 256
        with _lib.tuning(AH_SCAN_PACKED=1):
            packed = ds.distances(query=q)
            info = ds.packed_info()
        with _lib.tuning(AH_SCAN_PACKED=0):
            plain = ds.distances(query=q)
    ds.close()
    return packed, plain, want, info


@pytest.mark.parametrize("metric", [EUCLIDEAN, COSINE, DOT])
@pytest.mark.parametrize("kind", ["uniform", "normal", "clustered", "low_rank", "edge"])
@pytest.mark.parametrize("dims", [32, 96, 640, 768, 1536])
def test_packed_scan_bit_equal(metric, kind, dims):
    n = 3000
    vecs = rows(kind, n, dims, seed=dims * 7 + metric)
    q = np.random.default_rng(dims).standard_normal(dims).astype(np.float32)
    packed, plain, want, info = scan_both(metric, vecs, q)
    assert info["present"], "AH_SCAN_PACKED=1 made no packed copy"
    assert info["raw_rows"] < n
    if kind == "edge":
        assert info["raw_rows"] >= n // 7
    assert np.array_equal(bits(packed), bits(plain)), "packed scan differs from the f32 scan"
    assert np.array_equal(bits(packed), bits(want)), "packed scan differs from the oracle"


def test_packed_copy_lifecycle():
    """Not made below 64 Ki rows by default; made by the first scan over all rows, never by a gather; kept across
    ah_preprocess_dot (which writes the headers only)."""
    from arroy_amd import Dataset, _lib, distances
    from oracle import oracle as O
    n, dims = 1000, 64
    vecs = O.synth(3, 1, n, dims)
    ds = Dataset(distances.DotProduct, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    ds.preprocess_dot()
    ds.finalize()
    q = vecs[10]
    ds.distances(query=q)
    assert not ds.packed_info()["present"]  # automatic: too few rows
    with _lib.tuning(AH_SCAN_PACKED=1):
        ds.distances(query=q, ids=np.arange(0, n, 3, dtype=np.uint32))
        assert not ds.packed_info()["present"]  # a gather never makes it
        a = ds.distances(query=q)
        assert ds.packed_info()["present"]
        ds.preprocess_dot()
        assert ds.packed_info()["present"]
        b = ds.distances(query=q)
    assert np.array_equal(bits(a), bits(b))
    ds.close()


@pytest.mark.parametrize("dims,made", [(128, False), (768, True)])
def test_automatic_mode_packs_only_where_it_saves_bytes(dims, made):
    """AH_SCAN_PACKED=-1 from 64 Ki rows: at 128 dims a packed row (512 B + 2) is no smaller than the f32 row (512 B), so
    there is no copy; at 768 dims (2690 B of 3072) there is one, and the scan is the f32 rows' bit for bit."""
    from arroy_amd import Dataset, _lib, distances
    from oracle import oracle as O
    n = 65536
    vecs = O.synth(11, 1, n, dims)
    ds = Dataset(distances.Cosine, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    ds.finalize()
    assert _lib.tuning_get("AH_SCAN_PACKED")[0] == -1
    q = vecs[5]
    got = ds.distances(query=q)
    assert ds.packed_info()["present"] == made
    with _lib.tuning(AH_SCAN_PACKED=0):
        plain = ds.distances(query=q)
    assert np.array_equal(bits(got), bits(plain))
    ds.close()
