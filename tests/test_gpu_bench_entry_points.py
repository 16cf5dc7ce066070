"""The entry points only bench.py reached, or nothing: `ah_bench_scan` (its `out` array is what the benchmark samples to gate
the headline scan figure), `ah_bench_memcpy`, `ah_bench_read`, `ah_dataset_upload_flush`, `ah_group_upload_flush`,
`ah_group_size`, `ah_device_name`.  Values are compared in bits; times are only required to be positive and finite."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def staged(metric, dims, n, seed):
    from arroy_amd import Dataset, distances
    from oracle import oracle as O
    vecs = np.random.default_rng(seed).standard_normal((n, dims)).astype(np.float32)
    ds = Dataset(distances.BY_METRIC[metric], dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    od = O.Data(metric, vecs)
    if metric == 3:
        ds.preprocess_dot()
        od.preprocess_dot()
    return ds.finalize(), od, vecs


# ---- ah_bench_scan ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("dims", [32, 100])
def test_bench_scan_output_is_the_distance_scan(metric, dims):
    from arroy_amd import _lib
    n_rows, q = 3001, 7
    ds, od, vecs = staged(metric, dims, n_rows, seed=metric * 10 + dims)
    with _lib.tuning(AH_SCAN_PACKED=0):
        want = ds.distances(item=q)
    assert np.array_equal(bits(want), bits(od.distances(*od.item_leaf(q)))), "the reference scan is the oracle's"
    for packed in (0, 1):
        with _lib.tuning(AH_SCAN_PACKED=packed):
            for n in (1, n_rows - 1, n_rows):
                for it in (1, 3):
                    ms, out = ds.bench_scan(q, n, it, want_out=True)
                    assert out.shape == (n,) and np.array_equal(bits(out), bits(want[:n])), f"packed={packed} n={n} it={it}"
                    assert math.isfinite(ms) and ms > 0.0
            ms, out = ds.bench_scan(q, n_rows, 2)
            assert out is None and ms > 0.0
        # the packed instantiation ran exactly where there is a packed copy: the three metrics that have one, dims % 32 == 0
        assert ds.packed_info()["present"] == (packed == 1 and metric in (0, 2, 3) and dims % 32 == 0)
    ds.close()


def test_bench_scan_refuses_bad_arguments():
    from arroy_amd import ArroyHipError, Dataset, distances
    ds, od, vecs = staged(0, 32, 100, seed=1)
    for what, args in (("n == 0", (7, 0, 1)), ("n > len", (7, 101, 1)), ("iterations == 0", (7, 100, 0))):
        with pytest.raises(ArroyHipError) as e:
            ds.bench_scan(*args, want_out=True)
        assert e.value.status == INVALID_ARGUMENT, what
    fresh = Dataset(distances.Euclidean, 32, 4)
    fresh.upload_vectors(np.arange(4), vecs[:4])
    with pytest.raises(ArroyHipError) as e:
        fresh.bench_scan(0, 4, 1)
    assert e.value.status == 7, "not finalized"
    assert ds.bench_scan(7, 100, 1)[0] > 0.0
    fresh.close()
    ds.close()


# ---- ah_bench_memcpy / ah_bench_read: they run and refuse; no rate is asserted ---------------------------------------------

@pytest.mark.parametrize("probe", ["bench_memcpy", "bench_read"])
def test_bandwidth_probes_run_at_their_smallest_sizes(probe):
    from arroy_amd import ArroyHipError, _lib
    L = _lib.lib()
    fn, raw = {"bench_memcpy": (_lib.bench_memcpy, L.ah_bench_memcpy), "bench_read": (_lib.bench_read, L.ah_bench_read)}[probe]
    for nbytes in (4096, 1 << 20):
        for it in (1, 3):
            ms = fn(0, nbytes, it)
            assert math.isfinite(ms) and ms > 0.0, (probe, nbytes, it, ms)
    refused = [(0, 1), (4096, 0)] + ([(4095, 1)] if probe == "bench_read" else [])
    for nbytes, it in refused:
        with pytest.raises(ArroyHipError) as e:
            fn(0, nbytes, it)
        assert e.value.status == INVALID_ARGUMENT, (probe, nbytes, it)
    assert raw(0, 4096, 1, None) == INVALID_ARGUMENT, "a NULL output is refused"
    assert fn(0, 4096, 1) > 0.0


# ---- the rest ----------------------------------------------------------------------------------------------------------------

def test_upload_flush_waits_and_changes_nothing():
    from arroy_amd import Dataset, _lib, distances
    n, dims = 5000, 96
    vecs = np.random.default_rng(3).standard_normal((n, dims)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint32) * 3
    L = _lib.lib()
    flushed, plain = Dataset(distances.Cosine, dims, n), Dataset(distances.Cosine, dims, n)
    assert L.ah_dataset_upload_flush(flushed._h) == 0, "nothing staged yet: nothing to wait for"
    for ds in (flushed, plain):
        ds.upload_vectors(ids[: n // 2], vecs[: n // 2])
        if ds is flushed:
            assert L.ah_dataset_upload_flush(ds._h) == 0
        ds.upload_vectors(ids[n // 2:], vecs[n // 2:])
        if ds is flushed:
            assert L.ah_dataset_upload_flush(ds._h) == 0
            assert L.ah_dataset_upload_flush(ds._h) == 0, "twice in a row"
        ds.finalize()
    assert len(flushed) == len(plain) == n
    from oracle import oracle as O
    od = O.Data(2, vecs, ids=ids)
    want = od.distances(*od.item_leaf(11))
    assert np.array_equal(bits(flushed.distances(item=int(ids[11]))), bits(want))
    assert np.array_equal(bits(plain.distances(item=int(ids[11]))), bits(want))
    assert np.array_equal(flushed.read_headers(), plain.read_headers())
    assert np.array_equal(bits(flushed.item_vector(int(ids[n - 1]))), bits(vecs[n - 1]))
    assert L.ah_dataset_upload_flush(flushed._h) == 0, "after finalize: still only a wait"
    assert L.ah_dataset_upload_flush(None) == INVALID_ARGUMENT, "a NULL handle is refused"
    flushed.close()
    plain.close()


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_group_flush_and_size(devices):
    from arroy_amd import DatasetGroup, _lib, distances
    n, dims = 3000, 40
    vecs = np.random.default_rng(4).standard_normal((n, dims)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint32)
    L = _lib.lib()
    g = DatasetGroup(distances.Euclidean, dims, n, devices)
    size = C.c_uint32(99)
    assert L.ah_group_size(g._h, C.byref(size)) == 0 and size.value == len(devices) == len(g)
    g.flush()  # nothing staged yet
    g.upload_vectors(ids[:1000], vecs[:1000])
    g.flush()
    g.upload_vectors(ids[1000:], vecs[1000:])
    g.flush()
    g.flush()
    g.finalize()
    from oracle import oracle as O
    od = O.Data(0, vecs)
    want = od.distances(*od.item_leaf(5))
    for i in range(len(devices)):
        member = g.member(i)
        assert len(member) == n and np.array_equal(bits(member.distances(item=5)), bits(want)), f"member {i}"
    g.flush()
    assert L.ah_group_size(g._h, C.byref(size)) == 0 and size.value == len(devices)
    assert L.ah_group_size(None, C.byref(size)) == INVALID_ARGUMENT and L.ah_group_size(g._h, None) == INVALID_ARGUMENT
    assert L.ah_group_upload_flush(None) == INVALID_ARGUMENT
    g.close()


def test_device_name():
    import arroy_amd
    from arroy_amd import ArroyHipError, _lib
    name = arroy_amd.device_name(0)
    assert name.strip() and "CUs" in name, name
    buf = C.create_string_buffer(b"\x7f" * 8, 8)
    assert _lib.lib().ah_device_name(0, buf, 8) == 0 and len(buf.value) == 7 and name.startswith(buf.value.decode()), "truncated, terminated"
    assert _lib.lib().ah_device_name(0, None, 8) == INVALID_ARGUMENT and _lib.lib().ah_device_name(0, buf, 0) == INVALID_ARGUMENT
    with pytest.raises(ArroyHipError) as e:
        arroy_amd.device_name(arroy_amd.device_count() + 7)
    assert e.value.status == 3
    # the refusal is reported once: the launch checks of the next calls (staging, codec, scan) must not find it again
    ds, od, vecs = staged(0, 32, 64, seed=2)
    assert np.array_equal(bits(ds.distances(item=3)), bits(od.distances(*od.item_leaf(3))))
    ds.close()
