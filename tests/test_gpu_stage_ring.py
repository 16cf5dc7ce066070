"""The staging ring past its end (arroy_amd/csrc/stage.hip): uploads and updates of more chunks than the ring has slots, on a
dataset and on a device group, from f32 vectors and from stored records.

A chunk is sized from kStageBytes and the ring has kRing slots, so a call of more than kRing chunks reuses slot 0 and has to
wait for the transfers out of it; a second call starts wherever the first one stopped and wraps again.  Every test compares,
bit for bit, with a `Dataset` that staged the same items alone in ONE call: the headers, `distances(item=...)` over ALL rows
(every row of every chunk takes part) and the item vectors on both sides of every chunk boundary."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

from arroy_amd import Dataset, DatasetGroup  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

STAGE_BYTES = 32 << 20  # kStageBytes: what one ring slot holds of a call (rows or records, and their ids)
RING = 3                # kRing: the slots of a staging ring


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"


def vector_chunk(cls, dims):
    """Rows per chunk of upload_vectors: f32 rows at the staging pitch (whole 128-byte lines; 1-bit metrics: whole float4) + an id."""
    fpitch = (dims + 3) & ~3 if cls.metric >= 4 else (dims + 31) & ~31
    return STAGE_BYTES // (4 * fpitch + 4)


def record_chunk(cls, dims):
    """Records per chunk of upload_records (f32 metrics): the row re-pitched to whole lines + the header + an id."""
    return STAGE_BYTES // (4 * ((dims + 31) & ~31) + cls.header_size() + 4)


def two_calls(chunk):
    """Two calls of RING chunks each: the second starts on slot 0 while the events of the first are still pending."""
    a, b = (RING - 1) * chunk + chunk * 3 // 10, (RING - 1) * chunk + chunk // 10
    assert -(-a // chunk) == RING and -(-b // chunk) == RING
    return a, b


def long_call(chunk, total):
    """One call that runs past the ring (RING + 2 chunks, so it stops on slot 2), and the rest in a second one."""
    a = (RING + 1) * chunk + chunk // 8
    assert -(-a // chunk) == RING + 2 and a < total
    return a, total - a


def boundary_rows(calls, chunk):
    """First and last row of every chunk of every call."""
    rows, start = set(), 0
    for n in calls:
        for lo in range(0, n, chunk):
            rows |= {start + lo, start + min(n, lo + chunk) - 1}
        start += n
    return sorted(rows)


class World:
    """The vectors of a width, the datasets staged alone in one call, and the stored records: made once, left unchanged."""

    def __init__(self):
        self.vec, self.single, self.rec = {}, {}, {}

    def vectors(self, dims, n):
        if dims not in self.vec or len(self.vec[dims]) < n:
            self.vec[dims] = np.random.default_rng(dims).standard_normal((n, dims)).astype(np.float32)
        return self.vec[dims][:n]

    @staticmethod
    def ids(n):
        return np.arange(n, dtype=np.uint32) * 2 + 1  # not 0 .. n - 1: the id table path

    def alone(self, cls, dims, n):
        key = (cls.name, dims, n)
        if key not in self.single:
            ds = Dataset(cls, dims, n)
            ds.upload_vectors(self.ids(n), self.vectors(dims, n))
            self.single[key] = ds.finalize()
        return self.single[key]

    def records(self, cls, dims, n):
        key = (cls.name, dims, n)
        if key not in self.rec:
            oracle = O.Data(cls.metric, self.vectors(dims, n))
            self.rec[key] = [b"\0" + oracle.headers[i].tobytes() + oracle.codec[i].tobytes() for i in range(n)]
        return self.rec[key]

    def close(self):
        for ds in self.single.values():
            ds.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def assert_same(single, other, ids, rows):
    assert len(other) == len(single) == len(ids)
    assert other.read_headers().tobytes() == single.read_headers().tobytes()
    for q in (0, len(ids) // 2, len(ids) - 1):
        assert other.distances(item=int(ids[q])).tobytes() == single.distances(item=int(ids[q])).tobytes(), q
    for r in rows:
        assert other.item_vector(int(ids[r])).tobytes() == single.item_vector(int(ids[r])).tobytes(), r


def stage_group(cls, dims, devices, calls, ids, vecs=None, records=None):
    g = DatasetGroup(cls, dims, len(ids), devices)
    lo = 0
    for n in calls:
        if records is None:
            g.upload_vectors(ids[lo:lo + n], vecs[lo:lo + n])
        else:
            g.upload_records(ids[lo:lo + n], records[lo:lo + n])
        lo += n
    assert lo == len(ids)
    return g.finalize()


def check_group(g, single, ids, rows):
    for i in range(len(g)):
        assert_same(single, g.member(i), ids, rows)
    g.close()


N768 = sum(two_calls(vector_chunk(D.Cosine, 768)))  # (records of 768 dimensions: the same three chunks and three chunks)


@pytest.mark.parametrize("split", [two_calls, long_call], ids=["3+3_chunks", "5+1_chunks"])
def test_group_vectors_past_the_ring(world, split):
    cls, dims, n = D.Cosine, 768, N768
    chunk = vector_chunk(cls, dims)
    calls = split(chunk) if split is two_calls else split(chunk, n)
    ids, vecs = world.ids(n), world.vectors(dims, n)
    g = stage_group(cls, dims, [0, 0], calls, ids, vecs=vecs)
    check_group(g, world.alone(cls, dims, n), ids, boundary_rows(calls, chunk))


def test_group_records_past_the_ring(world):
    cls, dims, n = D.Euclidean, 768, N768
    chunk = record_chunk(cls, dims)
    calls = two_calls(vector_chunk(cls, dims))
    assert [-(-c // chunk) for c in calls] == [RING, RING]
    ids = world.ids(n)
    g = stage_group(cls, dims, [0, 0, 0], calls, ids, records=world.records(cls, dims, n))
    check_group(g, world.alone(cls, dims, n), ids, boundary_rows(calls, chunk))


def test_group_one_bit_vectors_past_the_ring(world):
    """The f32 chunk lands in the slot's piece of every member's device scratch and is quantised from there."""
    cls, dims, n = D.BinaryQuantizedCosine, 768, N768
    chunk = vector_chunk(cls, dims)
    calls = two_calls(chunk)
    ids, vecs = world.ids(n), world.vectors(dims, n)
    g = stage_group(cls, dims, [0, 0], calls, ids, vecs=vecs)
    check_group(g, world.alone(cls, dims, n), ids, boundary_rows(calls, chunk))


def test_dataset_records_past_the_ring(world):
    cls, dims, n = D.Euclidean, 768, N768
    chunk = record_chunk(cls, dims)
    calls = two_calls(vector_chunk(cls, dims))
    assert [-(-c // chunk) for c in calls] == [RING, RING]
    ids, records = world.ids(n), world.records(cls, dims, n)
    ds = Dataset(cls, dims, n)
    lo = 0
    for c in calls:
        ds.upload_records(ids[lo:lo + c], records[lo:lo + c])
        lo += c
    ds.finalize()
    assert_same(world.alone(cls, dims, n), ds, ids, boundary_rows(calls, chunk))
    ds.close()


def test_group_repitched_rows_past_the_ring(world):
    """70 dimensions travel at a pitch of 96 floats: the chunk is sized from the pitch, not from the width."""
    cls, dims = D.Euclidean, 70
    chunk = vector_chunk(cls, dims)
    assert chunk == STAGE_BYTES // (4 * 96 + 4)
    n = (RING + 1) * chunk + chunk // 8 + chunk // 2
    calls = long_call(chunk, n)
    ids, vecs = world.ids(n), world.vectors(dims, n)
    g = stage_group(cls, dims, [0, 0], calls, ids, vecs=vecs)
    check_group(g, world.alone(cls, dims, n), ids, boundary_rows(calls, chunk))


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["dataset", "group"])
def test_update_past_the_ring(world, devices):
    """update_vectors with upserted rows for RING + 2 chunks into a dataset of 3000 rows: replaced, new and removed ids."""
    cls, dims, n_old = D.Cosine, 768, 3000
    chunk = vector_chunk(cls, dims)
    n_up = (RING + 1) * chunk + chunk // 8
    vecs = world.vectors(dims, N768)
    assert n_up <= N768
    old_ids, old_vecs = np.arange(n_old, dtype=np.uint32) * 2, np.ascontiguousarray(vecs[:n_old, ::-1])  # (other rows than the new)
    up_ids, up_vecs = np.arange(n_up, dtype=np.uint32) + 1000, vecs[:n_up]  # even ids up to 5998 are replaced, the rest is new
    rm_ids = np.array([0, 2, 4, 7, 1000], dtype=np.uint32)  # 7 is absent, 1000 leaves and comes back
    kept = ~np.isin(old_ids, rm_ids) & ~np.isin(old_ids, up_ids)
    new_ids = np.concatenate([old_ids[kept], up_ids])
    order = np.argsort(new_ids)
    new_ids, new_vecs = new_ids[order], np.concatenate([old_vecs[kept], up_vecs])[order]
    key = ("updated", dims, len(new_ids))
    if key not in world.single:
        ds = Dataset(cls, dims, len(new_ids))
        ds.upload_vectors(new_ids, new_vecs)
        world.single[key] = ds.finalize()
    want = world.single[key]
    if devices is None:
        got = Dataset(cls, dims, n_old)
        got.upload_vectors(old_ids, old_vecs)
    else:
        got = DatasetGroup(cls, dims, n_old, devices)
        got.upload_vectors(old_ids, old_vecs)
    got.finalize()
    got.update_vectors(rm_ids, up_ids, up_vecs)
    # the rows of the upserted chunks' boundaries, wherever the merge put them
    rows = sorted({int(np.searchsorted(new_ids, up_ids[r])) for r in boundary_rows([n_up], chunk)} | {0, len(new_ids) - 1})
    for member in ([got] if devices is None else [got.member(i) for i in range(len(devices))]):
        assert_same(want, member, new_ids, rows)
    got.close()


def test_group_uploads_never_read_the_callers_memory_after_return(world):
    """The staging contract (include/arroy_hip.h) on a group: the pointers are not used after return, although the DMA of the
    last chunks to any member may still be in flight.  Overwrite the source right after every call; the members must hold the
    originals."""
    cls, dims, n = D.Cosine, 768, N768
    chunk = vector_chunk(cls, dims)
    calls = two_calls(chunk)
    ids, keep = world.ids(n), world.vectors(dims, n)
    g = DatasetGroup(cls, dims, n, [0, 0])
    lo = 0
    for c in calls:
        a, i = keep[lo:lo + c].copy(), ids[lo:lo + c].copy()
        g.upload_vectors(i, a)
        a[:] = np.nan
        i[:] = 0
        lo += c
    g.finalize()
    rows = boundary_rows(calls, chunk)
    for m in range(2):
        for r in rows:
            assert g.member(m).item_vector(int(ids[r])).tobytes() == keep[r].tobytes(), (m, r)
    check_group(g, world.alone(cls, dims, n), ids, rows)
