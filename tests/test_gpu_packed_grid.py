"""Grid rows of the packed copy on the device (AH_SCAN_GRID): the scan of a copy made with the switch on equals
the scan of one made with it off, the scan of the f32 rows (AH_SCAN_PACKED=0) and the oracle, bit for bit — three metrics,
dims 32 / 96 / 640 / 768 / 1536 (last groups of 1, 3, 4 and 8 blocks), datasets of grid rows only, of none, of every row form
at once, and of grid rows that the 28-bit rule leaves raw; with the default grid and with it capped (AH_SCAN_BLOCKS=8: the
grid-stride loop).  ah_dataset_packed_rows reports the grid rows the numpy rule of test_packed_grid_cpu counts, and after an
update of the dataset the counts are those of a fresh staging."""
import numpy as np
import pytest

from test_packed_grid_cpu import is_grid
from test_packed_rows_cpu import RAW, pack_row

pytestmark = pytest.mark.gpu

EUCLIDEAN, COSINE, DOT = 0, 2, 3
KINDS = ["all_grid", "none_grid", "mixed", "grid_raw28"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def grid_rows(n, dims, seed):
    """uniform[-1, 1) rows of the oracle's generator (multiples of 2^-23), the exact -1.0 (a 24th magnitude bit) taken out"""
    from oracle import oracle as O
    v = O.synth(seed, O.SYNTH_UNIFORM_PM1, n, dims)
    v[v == np.float32(-1.0)] = np.float32(0.5)
    v[:, 0] = np.float32(0.75)  # e_max = 126 in every row
    return v


def rows(kind, n, dims, seed):
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    if kind == "all_grid":
        return grid_rows(n, dims, seed)
    if kind == "none_grid":
        return rng.standard_normal((n, dims)).astype(np.float32)
    if kind == "grid_raw28":
        v = grid_rows(n, dims, seed)
        v[:, 5] = np.float32(2.0 ** -21)     # 20 binades below e_max: raw in the 28-bit rule, on the grid of 2^-23
        v[1::2, 9] = np.float32(-(2.0 ** -23))  # the unit itself, 22 binades down
        return v
    assert kind == "mixed"
    v = rng.standard_normal((n, dims)).astype(np.float32)  # plain rows
    v[0::8] = grid_rows(n, dims, seed)[0::8]               # grid
    g = O.synth(seed + 1, O.SYNTH_NORMAL, n, dims)          # grid (multiples of 2^-20), with +-0
    g[:, 3], g[:, 4] = 0.0, np.float32(-0.0)
    v[1::8] = g[1::8]
    v[2::8, :dims // 2] = 0.0                              # plain with exponent-0 elements (code 15)
    v[3::8, 5] *= np.float32(2.0 ** -20)                   # raw: a full-mantissa element far below the rest
    v[4::8] = grid_rows(n, dims, seed + 2)[4::8] * np.float32(2.0 ** 100)   # grid, huge
    v[5::8] = grid_rows(n, dims, seed + 3)[5::8] * np.float32(2.0 ** -100)  # grid, tiny (e_max = 26)
    v[6::8] = grid_rows(n, dims, seed + 4)[6::8] * np.float32(2.0 ** -102)  # e_max = 24: below the grid's range, plain
    v[7::8, 2] = np.float32(1e-40)                         # a denormal: plain
    v[7] = 0.0                                             # an all-zero row: plain
    return v


def expected_counts(vecs, grid_on):
    grid = sum(1 for r in vecs if is_grid(r)) if grid_on else 0
    raw = sum(1 for r in vecs if not (grid_on and is_grid(r)) and pack_row(r)[0] == RAW)
    return {"present": True, "raw_rows": raw, "grid_rows": grid}


def staged(metric, vecs):
    from arroy_amd import Dataset, distances
    n, dims = vecs.shape
    ds = Dataset(distances.BY_METRIC[metric], dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    if metric == DOT:
        ds.preprocess_dot()
    return ds.finalize()


@pytest.mark.parametrize("metric", [EUCLIDEAN, COSINE, DOT])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims", [32, 96, 640, 768, 1536])
def test_grid_scan_bit_equal(metric, kind, dims):
    from arroy_amd import _lib
    from oracle import oracle as O
    n = 1500
    vecs = rows(kind, n, dims, seed=dims * 11 + metric)
    q = np.random.default_rng(dims + 1).standard_normal(dims).astype(np.float32)
    od = O.Data(metric, vecs)
    if metric == DOT:
        od.preprocess_dot()
    qv, qh = od.query_leaf(q)
    want = od.distances(qv, qh)
    on, off = staged(metric, vecs), staged(metric, vecs)
    got = {}
    for blocks in (0, 8):  # the default grid; 8 blocks of 32 octets: the grid-stride loop
        with _lib.tuning(AH_SCAN_BLOCKS=blocks, AH_SCAN_PACKED=1):
            with _lib.tuning(AH_SCAN_GRID=1):
                got["on", blocks] = on.distances(query=q)    # (the first call makes the copy, under the switch's value then)
            with _lib.tuning(AH_SCAN_GRID=0):
                got["off", blocks] = off.distances(query=q)
        with _lib.tuning(AH_SCAN_BLOCKS=blocks, AH_SCAN_PACKED=0):
            got["f32", blocks] = on.distances(query=q)
    info_on, info_off = on.packed_rows(), off.packed_rows()
    assert on.packed_info() == {k: info_on[k] for k in ("present", "raw_rows")}
    on.close(), off.close()
    assert info_on == expected_counts(vecs, True), (info_on, kind)
    assert info_off == expected_counts(vecs, False), (info_off, kind)
    if kind in ("all_grid", "grid_raw28"):
        assert info_on["grid_rows"] == n and info_on["raw_rows"] == 0
    if kind == "grid_raw28":
        assert info_off["raw_rows"] == n
    if kind == "none_grid":
        assert info_on["grid_rows"] == 0
    if kind == "mixed":
        assert info_on["grid_rows"] >= n // 2 - 1 and info_on["raw_rows"] >= n // 8 and \
            n - info_on["grid_rows"] - info_on["raw_rows"] >= n // 4
    for key, d in got.items():
        bad = np.nonzero(bits(d) != bits(want))[0]
        assert bad.size == 0, f"scan {key} differs from the oracle in rows {bad[:8]} (of {bad.size})"


def test_grid_counts_after_update():
    """An update drops the copy; the next scan makes it again from the rows as they are now: the counts of a fresh staging."""
    from arroy_amd import _lib
    n, dims = 800, 96
    vecs = rows("mixed", n, dims, seed=77)
    ds = staged(COSINE, vecs)
    q = vecs[3]
    with _lib.tuning(AH_SCAN_PACKED=1):
        ds.distances(query=q)
        assert ds.packed_rows() == expected_counts(vecs, True)
        # plain rows over grid rows, grid rows over plain ones, some removed
        rng = np.random.default_rng(78)
        upsert = np.arange(0, 400, 5, dtype=np.uint32)
        new = np.where((upsert % 2 == 0)[:, None], rng.standard_normal((upsert.size, dims)).astype(np.float32),
                       grid_rows(upsert.size, dims, 79))
        remove = np.arange(401, 800, 7, dtype=np.uint32)
        ds.update_vectors(remove, upsert, new)
        assert not ds.packed_rows()["present"]
        after = vecs.copy()
        after[upsert] = new
        keep = np.setdiff1d(np.arange(n), remove)
        fresh = staged(COSINE, after[keep])
        a, b = ds.distances(query=q), fresh.distances(query=q)
        assert ds.packed_rows() == fresh.packed_rows() == expected_counts(after[keep], True)
        assert np.array_equal(bits(a), bits(b))
        with _lib.tuning(AH_SCAN_GRID=0):  # read when the copy is made: the copy that exists stays what it is
            assert np.array_equal(bits(ds.distances(query=q)), bits(a))
            assert ds.packed_rows() == expected_counts(after[keep], True)
    ds.close(), fresh.close()
