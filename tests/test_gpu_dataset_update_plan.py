"""The plan kernels of a dataset update (arroy_amd/csrc/update.hip) past one scan tile, one chunk of tile sums and one grid.

The exclusive scan of the keep flags works on tiles of 4096 flags (k_scan_tiles / k_scan_add), scans the tile sums in chunks of
1024 with a carry between them (k_scan_sums), and four kernels finish their work in a grid-stride loop: k_move_rows (8192 blocks
of 4 waves: 32 768 rows a pass), k_upsert_dest (4096 x 256 = 1 048 576 upserts a pass) and k_update_flags (65 536 x 256 =
16 777 216 rows a pass).  The cases of test_gpu_dataset_update.py stay below every one of these sizes but one; the cases here sit
on them:

  1. tile seams: n_old around one, two and three tiles, with keep flags that change at the seams; checked like the cases of
     test_gpu_dataset_update.py, against a dataset staged afresh (assert_same);
  2. the second pass of k_move_rows (old rows and staged rows) and of k_upsert_dest;
  3. the second and third chunk of k_scan_sums and the second pass of k_update_flags.

The large cases of 2 and 3 are checked against the CPU oracle (light_check): no forest is built on them."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

from arroy_amd import Dataset, DatasetGroup, _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from test_gpu_dataset_update import assert_same, fresh, gpu, random_change, update  # noqa: E402,F401 (gpu: autouse fixture)

TILE = 4096          # kScanTile: flags scanned by one block of k_scan_tiles
CHUNK = TILE * 1024  # rows whose tile sums k_scan_sums scans in one chunk
SEAM_SIZES = [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 1]
SEAM_DIMS = 64
WORLDS = ["identity", "sparse"]


# ---- 1. tile seams ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def seam_world():
    """Rows and sparse ascending ids for the largest seam size (+ 1: the identity world of the shift pattern starts at id 1);
    a smaller world is a prefix.  The sparse ids leave room below the first, between most neighbours and above the last."""
    rng = np.random.default_rng(100)
    n = SEAM_SIZES[-1] + 1
    vecs = rng.standard_normal((n, SEAM_DIMS)).astype(np.float32)
    sparse = np.sort(rng.choice(np.arange(16, 1 << 18), n, replace=False)).astype(np.int64)
    vecs.setflags(write=False), sparse.setflags(write=False)
    return vecs, sparse


def world_ids(seam_world, world, n, first=0):
    return np.arange(first, first + n, dtype=np.int64) if world == "identity" else seam_world[1][:n]


def merge_and_compare(dist, ids, vecs, change, rng, what):
    """A dataset staged with (ids, vecs), one update through the merge path, compared with a fresh staging of the result.
    `change`: (remove, upsert, vectors), or a function of the items that returns them."""
    items = {int(i): v for i, v in zip(ids, vecs)}
    a = fresh(dist, SEAM_DIMS, items)
    remove, upsert, up_vecs = change(items) if callable(change) else change
    merged = a.update_paths()["merged"]
    update(a, items, remove, upsert, up_vecs)
    assert a.update_paths()["merged"] == merged + 1, what
    b = fresh(dist, SEAM_DIMS, items)
    assert_same(a, b, items, rng, what=what)
    a.close(), b.close()


def varied_change(rng, world):
    """random_change plus, where the ids have room for them (the identity ids 0 .. n - 1 have room above only), one new id
    below every stored id, one between two neighbours and one above the last"""
    def change(items):
        present = np.array(sorted(items), dtype=np.int64)
        id_space = int(present[-1]) + 2000
        remove, upsert, _ = random_change(rng, items, SEAM_DIMS, id_space, 150, 120, 90, 20)
        forced = {int(present[-1]) + 1}
        if world == "sparse":
            gap = int(np.flatnonzero(np.diff(present) > 1)[len(present) // 2])  # a gap in the middle of the ids
            forced |= {int(present[0]) - 1, int(present[gap]) + 1}
        upsert = sorted(set(upsert) | forced)
        return remove, upsert, rng.standard_normal((len(upsert), SEAM_DIMS)).astype(np.float32)
    return change


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("n_old", SEAM_SIZES)
def test_tile_seams_cosine(seam_world, n_old, world):
    """Keep flags that change at the seams of the scan's tiles.  Reaches: k_scan_tiles / k_scan_add with two to four tiles
    and non-zero tile prefixes (n_old > 4096), k_scan_sums over up to four sums, zero sums among them."""
    rng = np.random.default_rng(n_old)
    ids = world_ids(seam_world, world, n_old)
    vecs = seam_world[0][:n_old]
    one = rng.standard_normal((1, SEAM_DIMS)).astype(np.float32)
    none = np.zeros((0, SEAM_DIMS), dtype=np.float32)
    # nothing removed, one new id below every stored id: every ins[r] is 1, every row shifts by one.  The identity ids
    # 0 .. n - 1 have nothing below them: there the dataset starts with the ids 1 .. n_old and ends as 0 .. n_old.
    shift_ids = world_ids(seam_world, world, n_old, first=1)
    merge_and_compare(D.Cosine, shift_ids, vecs, ([], [int(shift_ids[0]) - 1], one), rng, "one id below all")
    rows = np.arange(n_old)
    patterns = [
        ("first row of every tile", rows[::TILE]),
        ("last row of every tile", np.union1d(rows[TILE - 1::TILE], rows[-1:])),
        ("rows 4095 and 4096", rows[TILE - 1:TILE + 1]),
        ("the second tile", rows[TILE:2 * TILE]),
        ("all but the last row", rows[:-1]),
        ("all but row 4096", np.delete(rows, TILE) if n_old > TILE else rows),  # (no row 4096: nothing stays)
    ]
    for name, leave in patterns:
        if leave.size:  # (n_old = 4095 has no row 4095, n_old <= 4096 no second tile: nothing to remove, no merge)
            merge_and_compare(D.Cosine, ids, vecs, (ids[leave], [], none), rng, name)
    merge_and_compare(D.Cosine, ids, vecs, varied_change(rng, world), rng, "random change")


@pytest.mark.parametrize("n_old", SEAM_SIZES)
def test_tile_seams_dot_product(seam_world, n_old):
    """The most varied pattern with two header floats a row riding through k_move_rows (the headers of kept rows are those
    DotProduct's preprocess wrote; update() preprocesses again, as a Writer build does)."""
    rng = np.random.default_rng(1000 + n_old)
    for world in WORLDS:
        ids = world_ids(seam_world, world, n_old)
        merge_and_compare(D.DotProduct, ids, seam_world[0][:n_old], varied_change(rng, world), rng, f"{world} random change")


# ---- the check of the large cases ------------------------------------------------------------------------------------------

def merge_on_host(old_ids, old_vecs, remove, upsert, up_vecs):
    """What an update leaves, restated in numpy: (final ids, final rows, the ids that left for good).  All ids ascending."""
    n = old_ids.size

    def held(ids, among):  # which of `ids` are among the ascending `among`, and where
        at = np.minimum(np.searchsorted(among, ids), max(among.size - 1, 0))
        found = among[at] == ids if among.size else np.zeros(ids.size, dtype=bool)
        return found, at[found]

    removed, rows = held(remove, old_ids)
    kept = np.ones(n, dtype=bool)
    kept[rows] = False
    kept[held(upsert, old_ids)[1]] = False
    keep_ids = old_ids[kept]
    to = np.searchsorted(keep_ids, upsert) + np.arange(upsert.size)  # the upserted ids merged into the kept ones
    from_old = np.ones(keep_ids.size + upsert.size, dtype=bool)
    from_old[to] = False
    final_ids = np.empty(from_old.size, dtype=np.uint32)
    final_ids[from_old], final_ids[to] = keep_ids, upsert
    final_vecs = np.empty((from_old.size, old_vecs.shape[1]), dtype=np.float32)
    final_vecs[from_old], final_vecs[to] = old_vecs[kept], up_vecs
    assert final_ids.size < 2 or (final_ids[1:] > final_ids[:-1]).all()
    gone = remove[removed]
    return final_ids, final_vecs, gone[~held(gone, upsert)[0]]


def seam_rows(n):
    """the first and the last row of tiles 0, 1, 1023, 1024 and the last tile of n rows (those that exist)"""
    last_tile = (n - 1) // TILE
    rows = set()
    for t in (0, 1, 1023, 1024, last_tile):
        if t <= last_tile:
            rows |= {t * TILE, min((t + 1) * TILE, n) - 1}
    return sorted(rows)


def light_check(a, old_ids, final_ids, final_vecs, gone, rng, what, full=True):
    """`a` against the oracle on (final_ids, final_vecs): its length, every row in its place (the full scan), the ids and
    their table (the gathered scan, item_vector, MissingKey), the headers.  full=False: the length and the full scan only."""
    n = final_ids.size
    assert len(a) == n, what
    oracle = O.Data(O.EUCLIDEAN, final_vecs, ids=final_ids)
    q = rng.standard_normal(final_vecs.shape[1]).astype(np.float32)
    qv, qh = oracle.query_leaf(q)
    want = oracle.distances(qv, qh)
    got = a.distances(query=q)
    assert got.tobytes() == want.tobytes(), (what, "rows differ at", np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
    if not full:
        return
    assert a.distances(query=q, ids=final_ids[::97]).tobytes() == want[::97].tobytes(), what
    headers = a.read_headers()
    assert headers.shape == (n, 1), what
    assert headers.tobytes() == oracle.headers.tobytes(), what
    # ~32 ids: the rows at the seams of the old and of the new dataset, and random ones
    some = rng.choice(final_ids, min(n, 20), replace=False)
    probe = np.concatenate([old_ids[seam_rows(old_ids.size)], final_ids[seam_rows(n)], some, gone[:4]])
    checked = 0
    for i in np.unique(probe):
        r = int(np.searchsorted(final_ids, i))
        if r < n and final_ids[r] == i:
            assert a.item_vector(int(i)).tobytes() == final_vecs[r].tobytes(), (what, int(i))
            checked += 1
        else:
            with pytest.raises(_lib.MissingKey):
                a.item_vector(int(i))
    assert checked >= some.size, what
    for i in gone[:: max(1, gone.size // 4)][:5]:
        with pytest.raises(_lib.MissingKey):
            a.item_vector(int(i))


def staged(ids, vecs, capacity=None):
    a = Dataset(D.Euclidean, vecs.shape[1], ids.size if capacity is None else capacity)
    a.upload_vectors(ids, vecs)
    return a.finalize()


# ---- 2. past one grid of k_move_rows and of k_upsert_dest ------------------------------------------------------------------

def test_merge_40k_second_pass_over_old_rows():
    """40 000 old rows, 5 % removed, new ids between them: k_move_rows goes round its stride loop twice over the old rows
    (32 768 rows a pass); ten tiles in k_scan_tiles / k_scan_add."""
    rng = np.random.default_rng(200)
    n, dims = 40_000, 4
    ids = 3 * np.arange(n, dtype=np.int64) + 1
    items = {int(i): v for i, v in zip(ids, rng.standard_normal((n, dims)).astype(np.float32))}
    a = fresh(D.Euclidean, dims, items)
    remove = rng.choice(ids, n // 20, replace=False)
    new = np.union1d(3 * rng.choice(n, 2000, replace=False) + 2, [0, int(ids[-1]) + 5])  # between, below, above
    upsert = np.union1d(new, rng.choice(ids, 500, replace=False))
    update(a, items, remove, upsert, rng.standard_normal((upsert.size, dims)).astype(np.float32))
    assert a.update_paths() == {"in_place": 0, "appended": 0, "merged": 1}
    b = fresh(D.Euclidean, dims, items)
    assert_same(a, b, items, rng, what="40k merge")
    a.close(), b.close()


@pytest.fixture(scope="module")
def rows_1_2m():
    rng = np.random.default_rng(201)
    n = 1_200_000
    vecs = rng.standard_normal((n, 4), dtype=np.float32)
    ids = 2 * np.arange(n, dtype=np.uint32)
    vecs.setflags(write=False), ids.setflags(write=False)
    return ids, vecs


def test_in_place_1_1m_replacements(rows_1_2m):
    """1 100 000 of 1 200 000 rows replaced: k_upsert_dest (1 048 576 upserts a pass) and the staged half of k_move_rows
    (32 768 rows a pass) go round their stride loops more than once."""
    rng = np.random.default_rng(202)
    ids, vecs = rows_1_2m
    a = staged(ids, vecs)
    at = np.sort(rng.choice(ids.size, 1_100_000, replace=False))
    up_vecs = rng.standard_normal((at.size, 4), dtype=np.float32)
    a.update_vectors([], ids[at], up_vecs)
    assert a.update_paths() == {"in_place": 1, "appended": 0, "merged": 0}
    final_vecs = vecs.copy()
    final_vecs[at] = up_vecs
    absent = ids[:: ids.size // 4] + np.uint32(1)
    light_check(a, ids, ids, final_vecs, absent, rng, "in place")
    a.close()


def test_append_1_1m_new_ids(rows_1_2m):
    """1 100 000 new ids above the last of 1 200 000, room reserved: the append path of k_upsert_dest and the staged half of
    k_move_rows past one grid."""
    rng = np.random.default_rng(203)
    ids, vecs = rows_1_2m
    n_new = 1_100_000
    a = staged(ids, vecs, capacity=ids.size + n_new)
    new = ids[-1] + np.uint32(1) + 2 * np.arange(n_new, dtype=np.uint32)
    up_vecs = rng.standard_normal((n_new, 4), dtype=np.float32)
    a.update_vectors([], new, up_vecs)
    assert a.update_paths() == {"in_place": 0, "appended": 1, "merged": 0}
    absent = np.concatenate([ids[:: ids.size // 2] + np.uint32(1), new[-2:] + np.uint32(1)])
    light_check(a, ids, np.concatenate([ids, new]), np.concatenate([vecs, up_vecs]), absent, rng, "append")
    a.close()


def test_merge_1_2m_without_an_id_table(rows_1_2m):
    """A merge that leaves an id near 2^31 on top of 1.2M rows: the ids span too much for an id -> row table (lut_len 0), so
    the gathered scan and item_vector find their rows by binary search in the ids k_move_rows wrote (every other large case
    here has dense ids and goes through the rebuilt table).  293 tiles; k_move_rows strides 37 times."""
    rng = np.random.default_rng(204)
    ids, vecs = rows_1_2m
    remove = ids[np.flatnonzero(rng.random(ids.size) < 0.01)]
    upsert = np.union1d(rng.integers(0, 2 * ids.size, 3000), [(1 << 31) + 7]).astype(np.uint32)
    up_vecs = rng.standard_normal((upsert.size, 4), dtype=np.float32)
    a = staged(ids, vecs)
    a.update_vectors(remove, upsert, up_vecs)
    assert a.update_paths() == {"in_place": 0, "appended": 0, "merged": 1}
    final_ids, final_vecs, gone = merge_on_host(ids, vecs, remove, upsert, up_vecs)
    light_check(a, ids, final_ids, final_vecs, gone, rng, "1.2M rows, top id past 2^31")
    a.close()


# ---- 3. past one chunk of k_scan_sums, past the grid of k_update_flags -----------------------------------------------------

N_FLAGS_GRID = (1 << 24) + 4097  # one tile and a row past the 65 536 x 256 threads of k_update_flags


@pytest.fixture(scope="module")
def rows_16m():
    """Rows for the largest case (268 MB); a smaller case takes a prefix.  The ids are the even numbers, so that new ids fit
    between any two."""
    vecs = np.random.default_rng(300).standard_normal((N_FLAGS_GRID, 4), dtype=np.float32)
    vecs.setflags(write=False)
    return vecs


def chunk_change(rng, pattern, ids):
    """The removals of `pattern` and a few thousand upserts spread over the id range (ids present: replaced, or taken back if
    also removed; odd ids: new between two rows; ids above the last).  The last old row always stays: it is the only row of
    the last tile at 4096 * k + 1 rows, and its place is the total of every tile before it (with exactly 1024 tiles, "carry0"
    removes it with its tile, and "carrymax" has no tile past the first chunk: there about half of tile 1023 goes; with 1025
    tiles the last row is all there is past the first chunk, so "carrymax" removes nothing and the upserts alone make the merge:
    the carry is then the whole first chunk)."""
    n = ids.size
    last = ids[-1]
    if pattern == "random":  # about 1 %
        remove = ids[np.flatnonzero(rng.random(n) < 0.01)]
        remove = remove[remove != last]
    elif pattern == "carry0":  # every row of tiles 0 .. 1023 goes: the carry into the second chunk is 0
        remove = ids[:CHUNK]
    else:  # "carrymax": tiles 0 .. 1023 stay, about half of the rest goes: the carry is as large as it can be
        rest = CHUNK if n > CHUNK else CHUNK - TILE
        remove = ids[rest + np.flatnonzero(rng.random(n - rest) < 0.5)]
        remove = remove[remove != last]
    upsert = np.unique(rng.integers(0, 2 * n + 2000, 3000)).astype(np.uint32)
    upsert = upsert[upsert != last]
    return remove, upsert, rng.standard_normal((upsert.size, 4), dtype=np.float32)


@pytest.mark.parametrize("pattern", ["random", "carry0", "carrymax"])
@pytest.mark.parametrize("n_old", [CHUNK, CHUNK + 1, 2 * CHUNK + 1], ids=["1024 tiles", "1025 tiles", "2049 tiles"])
def test_scan_sums_chunks(rows_16m, n_old, pattern):
    """1024 tiles are exactly one chunk of k_scan_sums, 1025 the first size with a second chunk (carry, wave_sums used again),
    2049 take three.  k_scan_add adds prefixes up to the whole dataset; k_move_rows strides some hundred times.
    Seconds on the MI355X (limit: twice test_updates_equal_a_fresh_staging[cosine-768], 0.24 to 0.28): 1024 tiles 0.16 / 0.33 /
    0.14, 1025 tiles 0.17 / 0.33 / 0.14, 2049 tiles 0.37 / 0.71 / 0.56 (random / carry0 / carrymax).  The five over the limit
    spend most of it inside update_vectors (0.41 of 0.75 s at 2049 tiles, carry0: the plan looks up each of 4M removed ids on
    the host) and in upload_vectors (0.11 s); the numpy merge takes 0.19 s and the whole check 0.04 s."""
    rng = np.random.default_rng(n_old % 1000 + len(pattern))
    ids, vecs = 2 * np.arange(n_old, dtype=np.uint32), rows_16m[:n_old]
    remove, upsert, up_vecs = chunk_change(rng, pattern, ids)
    a = staged(ids, vecs)
    a.update_vectors(remove, upsert, up_vecs)
    assert a.update_paths() == {"in_place": 0, "appended": 0, "merged": 1}
    final_ids, final_vecs, gone = merge_on_host(ids, vecs, remove, upsert, up_vecs)
    light_check(a, ids, final_ids, final_vecs, gone, rng, f"{n_old} rows, {pattern}")
    a.close()


def test_scan_sums_chunks_group(rows_16m):
    """A chunk case through a DatasetGroup (one device listed twice): every member is planned before any is committed."""
    rng = np.random.default_rng(301)
    n_old = CHUNK + 1
    ids, vecs = 2 * np.arange(n_old, dtype=np.uint32), rows_16m[:n_old]
    remove, upsert, up_vecs = chunk_change(rng, "random", ids)
    g = DatasetGroup(D.Euclidean, 4, n_old, [0, 0])
    g.upload_vectors(ids, vecs)
    g.finalize()
    g.update_vectors(remove, upsert, up_vecs)
    final_ids, final_vecs, gone = merge_on_host(ids, vecs, remove, upsert, up_vecs)
    for i in range(2):
        assert g.member(i).update_paths() == {"in_place": 0, "appended": 0, "merged": 1}
        light_check(g.member(i), ids, final_ids, final_vecs, gone, rng, f"member {i}")
    g.close()


def test_update_flags_second_pass(rows_16m):
    """2^24 + 4097 rows: k_update_flags (16 777 216 rows a pass) goes round twice; 4098 tiles, five chunks of k_scan_sums.
    Reduced to the length and the full scan against the oracle: with the gathered scan, the headers and the sampled ids it took
    0.69 s on the MI355X, against a limit of 0.24 to 0.28 s (twice test_updates_equal_a_fresh_staging[cosine-768], 0.12 and
    0.14 s in two runs).  Reduced it still takes 0.67 s: staging and update_vectors itself are most of it."""
    rng = np.random.default_rng(302)
    ids, vecs = 2 * np.arange(N_FLAGS_GRID, dtype=np.uint32), rows_16m
    remove, upsert, up_vecs = chunk_change(rng, "random", ids)
    a = staged(ids, vecs)
    a.update_vectors(remove, upsert, up_vecs)
    assert a.update_paths() == {"in_place": 0, "appended": 0, "merged": 1}
    final_ids, final_vecs, gone = merge_on_host(ids, vecs, remove, upsert, up_vecs)
    light_check(a, ids, final_ids, final_vecs, gone, rng, "2^24 + 4097 rows", full=False)
    a.close()
