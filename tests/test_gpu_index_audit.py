"""ah_index_audit / ah_forest_view_audit against the model of tests/audit_model.py: every assertion is `device report == model
report`, field for field (with a structure violation: the fields the header promises), and the per-tree stats equal
`TreeStore.stats`.  Datasets: 200 rows x 8 dimensions with ids 0 .. 199 (200 is no multiple of 32: the tail mask of the compare
pass; row_of_id is the identity), the sparse ids 7 i + 3 plus 0xFFFFFFFF (row_of_id searches the id array), and 33 rows with
sparse ids (row_of_id through the table).  No test provokes a fault: every broken input is one the audit is specified to
count."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import audit_model as M  # noqa: E402
from arroy_amd import Dataset, Index, _lib, audit_view  # noqa: E402
from arroy_amd import distances as D  # noqa: E402
from arroy_amd import index as I  # noqa: E402

from test_gpu_faults import DEVICE, OK, OOM, sweep  # noqa: E402
from test_gpu_index_delete import clone, host_delete, refused, same_store  # noqa: E402

NONE = 0xFFFFFFFF
DIMS = 8
DIST = D.Euclidean
COVER_MB = "AH_AUDIT_COVER_MB"


class World:
    def __init__(self, ids, seed=3):
        import arroy_amd
        assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
        self.ids = [int(i) for i in ids]
        self.vecs = np.random.default_rng(seed).standard_normal((len(self.ids), DIMS)).astype(np.float32)
        self.ds = Dataset(DIST, DIMS, len(self.ids))
        self.ds.upload_vectors(np.array(self.ids, dtype=np.uint32), self.vecs)
        self.ds.finalize()

    def close(self):
        _lib.tuning_set("AH_FAIL_ALLOC_AFTER", 0)
        self.ds.close()


@pytest.fixture(scope="module")
def dense():
    w = World(range(200))
    yield w
    w.close()


@pytest.fixture(scope="module")
def sparse():
    w = World([7 * i + 3 for i in range(199)] + [NONE])
    yield w
    w.close()


@pytest.fixture(scope="module")
def sparse33():
    w = World([7 * i + 3 for i in range(33)])
    yield w
    w.close()


def index_report(w, ix, trees=True):
    """the device's report of a resident index and the model's over its export"""
    got = ix.audit(trees=trees)
    want = M.model_of_export(ix.export(normals=False), w.ids, ix.export_info()["n_normals"], trees=trees)
    return got, want


def check_case(w, case, stats_of_store=True):
    """A case ah_index_create_from_view accepts: ah_index_audit == the model over the export == ah_forest_view_audit == the
    model over the view; -> the report"""
    view, keep = case.view(DIST, DIMS)
    ix = Index(w.ds, None, view=view)
    try:
        got, want = index_report(w, ix)
        assert got == want, (got, want)
        assert ix.audit() == {k: v for k, v in want.items() if k != "tree_stats"}
        assert ix.tree_stats() == want["tree_stats"]
    finally:
        ix.close()
    assert audit_view(w.ds, view, trees=True) == got
    assert case.model(w.ids, trees=True) == got
    if stats_of_store:
        assert M.plain_stats(got) == M.store_stats(case.store())
    return got


# ---- 1. the catalogue ---------------------------------------------------------------------------------------------------------

CATALOGUE = ["valid", "missing", "duplicate", "duplicate_across_trees", "unsorted", "floating", "deep_chain", "zero_trees",
             "zero_trees_with_nodes"]


@pytest.mark.parametrize("name", CATALOGUE)
def test_catalogue(dense, name):
    cases = M.catalogue(dense.ids)
    assert sorted(cases) == sorted(CATALOGUE)
    r = check_case(dense, cases[name])
    assert r["valid"] == int(name in ("valid", "duplicate_across_trees", "deep_chain", "zero_trees"))
    if name == "missing":
        assert (r["missing"], r["first_missing_tree"], r["first_missing_id"]) == (1, 1, 100)
    if name == "duplicate":
        assert (r["duplicate"], r["first_duplicate_tree"], r["first_duplicate_id"]) == (1, 0, 100)
    if name == "unsorted":
        assert r["unsorted"] == 3
    if name == "floating":
        assert (r["floating"], r["first_node"]["floating"]) == (3, 11)
    if name == "deep_chain":
        assert r["tree_stats"][0]["depth"] == 40
    if name.startswith("zero_trees"):
        assert all(r[c] == 0 for c in M.CLASSES if c != "floating") and r["floating"] == (4 if name.endswith("nodes") else 0)


def test_foreign_ids(dense, sparse, sparse33):
    r = check_case(dense, M.foreign_cases(dense.ids, [200, NONE]))
    assert (r["foreign"], r["valid"]) == (2, 0)
    r = check_case(sparse, M.foreign_cases(sparse.ids, [4, 11, NONE - 1]))  # ids in gaps of the sparse dataset
    assert (r["foreign"], r["valid"]) == (3, 0)
    r = check_case(sparse, M.foreign_cases(sparse.ids, []))  # 0xFFFFFFFF where it is stored
    assert r["valid"] == 1
    r = check_case(sparse33, M.foreign_cases(sparse33.ids, [NONE, 5]))  # ... and where it is not
    assert (r["foreign"], r["valid"]) == (2, 0)


def test_33_rows_and_the_sparse_catalogue(sparse, sparse33):
    """33 rows: two coverage words a tree, one bit in the last"""
    for w in (sparse33, sparse):
        cases = M.catalogue(w.ids) if len(w.ids) >= 200 else {
            "valid": M.Case([w.ids, (w.ids[:16], w.ids[16:]), (w.ids[:32], w.ids[32:], None)]),
            "missing": M.Case([w.ids[:32], (w.ids[:16], w.ids[17:])]),
            "duplicate": M.Case([(w.ids[:17], w.ids[16:]), w.ids]),
        }
        for name in ("valid", "missing", "duplicate"):
            r = check_case(w, cases[name])
            assert r["valid"] == int(name == "valid"), (name, r)
    r = check_case(sparse33, M.Case([sparse33.ids[:32], (sparse33.ids[:16], sparse33.ids[17:])]))
    assert (r["missing"], r["first_missing_tree"], r["first_missing_id"]) == (2, 0, sparse33.ids[32])


# ---- 2. structures ah_index_create_from_view refuses: the view audit returns and counts ------------------------------------------

BROKEN = ["two_parents", "root_is_a_child", "root_named_twice", "self_loop", "cycle_through_an_ancestor", "child_out_of_range",
          "root_out_of_range", "bad_kind", "bad_kind_root", "list_beyond_the_blob", "normal_beyond_the_blob"]


@pytest.mark.parametrize("name", BROKEN)
def test_broken_structures_are_counted_not_refused(dense, name):
    cases = M.broken(dense.ids)
    assert sorted(cases) == sorted(BROKEN)
    case = cases[name]
    view, keep = case.view(DIST, DIMS)
    with pytest.raises(_lib.ArroyHipError):  # (no index of it ever exists)
        Index(dense.ds, None, view=view)
    got = audit_view(dense.ds, view, trees=True)
    want = case.model(dense.ids, trees=True)
    assert M.structure_part(got) == M.structure_part(want), (got, want)
    assert got["valid"] == 0 and sum(got[c] for c in M.STRUCTURE) > 0
    assert audit_view(dense.ds, view)["valid"] == 0


# ---- 3. the contracts, on a resident index ----------------------------------------------------------------------------------------

def index_of(w, store):
    view, keep = store.to_view(DIST, DIMS)
    return Index(w.ds, None, view=view), keep[4]


def test_a_delete_the_dataset_did_not_follow(dense):
    case = M.catalogue(dense.ids)["valid"]
    store = case.store(DIST, DIMS)
    ix, dense_map = index_of(dense, store)
    try:
        gone = [0, 1, 64, 65, 199] + list(range(130, 160))
        got_store = clone(store)
        got_store.apply_delta(ix.delete_items(np.array(sorted(gone), dtype=np.uint32), 4), dense_map)
        same_store(got_store, host_delete(store, gone, 4))
        got, want = index_report(dense, ix)
        assert got == want, (got, want)
        assert got["missing"] == len(gone) * len(store.roots) and got["nodes_in_use"] < len(store.nodes)  # free slots: no finding
        assert all(got[c] == 0 for c in M.CLASSES if c != "missing")
        assert M.plain_stats(got) == M.store_stats(got_store)
        assert [t["root"] for t in got["tree_stats"]] == [dense_map[r] for r in got_store.roots]
    finally:
        ix.close()


def test_a_graft_whose_ids_are_not_the_replaced_nodes(dense):
    ids = dense.ids
    store = M.Case([(ids[:100], ids[100:]), ids]).store(DIST, DIMS)
    ix, _ = index_of(dense, store)
    try:
        # in place of the leaf ids[100:] (node 1): a sub-tree without id 150 and with id 7, which the other leaf holds
        sub = M.Case([(ids[100:150] + ids[151:180], [7] + ids[180:])])
        view, keep = sub.view(DIST, DIMS)
        ix.graft(view, [1])
        got, want = index_report(dense, ix)
        assert got == want, (got, want)
        assert (got["duplicate"], got["first_duplicate_tree"], got["first_duplicate_id"]) == (1, 0, 7)
        assert (got["missing"], got["first_missing_tree"], got["first_missing_id"]) == (1, 0, 150)
        assert got["unsorted"] == 0 and got["tree_stats"][0]["split_nodes"] == 2
    finally:
        ix.close()


def test_an_update_the_index_did_not_follow_then_followed_then_compacted():
    w = World(range(200), seed=5)
    try:
        store = M.catalogue(w.ids)["valid"].store(DIST, DIMS)
        ix, dense_map = index_of(w, store)
        removed = [3, 64, 100, 101, 199]
        ix.suspend()
        refused(lambda: ix.audit(), "suspended")
        w.ds.update_vectors(removed, [], None)
        ix.resume()
        w.ids = [i for i in w.ids if i not in removed]
        # (no search is issued in this state: the index holds ids that are no rows)
        got, want = index_report(w, ix)
        assert got == want, (got, want)
        assert got["foreign"] == len(removed) * len(store.roots) and got["n_items"] == 195
        assert all(got[c] == 0 for c in M.CLASSES if c != "foreign")
        after = clone(store)
        after.apply_delta(ix.delete_items(np.array(removed, dtype=np.uint32), 4), dense_map)
        got, want = index_report(w, ix)
        assert got == want and got["valid"] == 1, (got, want)
        assert M.plain_stats(got) == M.store_stats(after)
        before = got
        stats = ix.compact()
        assert stats["moved"] == 1
        got, want = index_report(w, ix)
        assert got == want and got["valid"] == 1
        assert M.plain_stats(got) == M.plain_stats(before) and got["nodes_in_use"] == before["nodes_in_use"] == stats["nodes_after"]
        assert ix.search(3, queries=w.vecs[:2], search_k=50)[0][0][0] == 0  # (valid: it may be searched again)
    finally:
        ix.close()
        w.close()


# ---- 4. tree groups ---------------------------------------------------------------------------------------------------------------

def test_tree_groups_give_identical_reports(dense, sparse33):
    ids = dense.ids
    five = {
        "valid": M.Case([ids, M.spread(ids, [0, 1, 63, 64, 65]), (ids[:100], ([], ids[100:]), None), (ids[:130], ids[130:]), M.chain(ids, 5)]),
        "missing": M.Case([ids, (ids[:100], ids[101:]), ids[1:], (ids[:31] + ids[33:], []), (ids[:199], [])]),
        "duplicate": M.Case([(ids[:101], ids[100:]), ids, ids, (ids[:32], ids[31:]), ([0, 5, 199], ids)]),
    }
    for name, case in five.items():
        assert len(case.roots) == 5
        reports = []
        for mb in (0, 64):
            with _lib.tuning(**{COVER_MB: mb}):
                reports.append(check_case(dense, case))
        assert reports[0] == reports[1], name
        assert reports[0]["valid"] == int(name == "valid")
    assert (five["missing"].model(ids)["missing"], five["duplicate"].model(ids)["duplicate"]) == (5, 5)
    with _lib.tuning(AH_AUDIT_COVER_MB=0):
        r = check_case(sparse33, M.Case([sparse33.ids[:32], (sparse33.ids[:16], sparse33.ids[17:]), sparse33.ids]))
    assert (r["missing"], r["first_missing_tree"], r["first_missing_id"]) == (2, 0, sparse33.ids[32])


# ---- 5. random forests with injected faults ------------------------------------------------------------------------------------------

def test_fifty_random_forests(dense, sparse):
    seen = set()
    for seed in range(50):
        w = (dense, sparse)[seed % 2]
        case = M.random_case(seed, w.ids)
        assert len(case.roots) <= 6 and len(case.nodes) <= 300
        want = case.model(w.ids, trees=True)
        view, keep = case.view(DIST, DIMS)
        with _lib.tuning(**{COVER_MB: (64, 0)[(seed // 2) % 2]}):
            if seed % 4 < 2:
                ix = Index(w.ds, None, view=view)
                try:
                    got = ix.audit(trees=True)
                finally:
                    ix.close()
            else:
                got = audit_view(w.ds, view, trees=True)
        assert got == want, (seed, got, want)
        assert M.plain_stats(got) == M.store_stats(case.store())
        seen.update(c for c in M.CLASSES if got[c])
    assert {"unsorted", "foreign", "duplicate", "missing"} <= seen and not seen & set(M.STRUCTURE)


# ---- 6. a fuzz round in the shape of the reference's examples/fuzz.rs ------------------------------------------------------------------

def test_six_incremental_builds_audit_themselves():
    n0, dims = 2000, 16
    g = np.random.default_rng(9)
    db = I.Database(D.Euclidean)
    w = I.Writer(db, 0, dims)
    st = w._st
    for i in range(n0):
        w.add_item(i, g.standard_normal(dims).astype(np.float32))
    next_id = n0
    try:
        for k in range(7):  # the first build is a full one
            if k:
                alive = sorted(st.items)
                for i in g.choice(alive, int(g.integers(1, 120)), replace=False):
                    w.del_item(int(i))
                for _ in range(int(g.integers(1, 160))):  # new items and new vectors for old ones
                    i = next_id if g.random() < 0.6 else int(g.choice(alive))
                    next_id += int(i == next_id)
                    w.add_item(i, g.standard_normal(dims).astype(np.float32))
            b = w.builder(random.Random(70 + k)).n_trees(4)
            b.device_audit = True
            b.build()  # (raises AssertionError on a finding or on stats that differ from the store's)
            reader = I.Reader.open(db, 0)
            reader.assert_validity()
            report = st.index.audit(trees=True)
            assert report["valid"] == 1 and report["n_items"] == len(st.items) and report["n_trees"] == 4
            assert M.plain_stats(report) == reader.stats()["tree_stats"]
        assert st.device_inserts >= 1 and st.device_deletes >= 1  # the resident index served builds, not only fresh uploads
        # a finding raises: the store's view with an id taken out of one list
        victim = next(nid for nid, nd in st.trees.nodes.items() if nd[0] == "D" and len(nd[1]) > 1)
        st.trees.nodes[victim] = ("D", st.trees.nodes[victim][1][1:])
        st.index.close()
        st.index = None
        with pytest.raises(AssertionError, match="missing 1"):
            reader.assert_validity()
    finally:
        if st.index is not None:
            st.index.close()
        if st.dataset is not None:
            st.dataset.close()


# ---- 7. allocation failures and refusals ---------------------------------------------------------------------------------------------

def test_audits_survive_every_allocation_failure(dense):
    case = M.catalogue(dense.ids)["missing"]
    view, keep = case.view(DIST, DIMS)
    want = case.model(dense.ids, trees=True)
    ix = Index(dense.ds, None, view=view)
    try:
        seen = sweep(lambda: ix.audit(trees=True))
        assert len(seen) >= 2 and set(seen) <= {OK, DEVICE, OOM} and OOM in seen, seen  # the scratch, the coverage words, the host's vectors
        assert ix.audit(trees=True) == want
        seen = sweep(lambda: audit_view(dense.ds, view, trees=True))
        assert len(seen) >= 5 and set(seen) <= {OK, DEVICE, OOM} and OOM in seen, seen  # ... and the copies of nodes, roots and ids
        assert audit_view(dense.ds, view, trees=True) == want
    finally:
        ix.close()


def test_refusals(dense):
    L = _lib.lib()
    case = M.catalogue(dense.ids)["valid"]
    view, keep = case.view(DIST, DIMS)
    ix = Index(dense.ds, None, view=view)
    try:
        rep = _lib.AhIndexAuditReport()
        rep.valid = 77
        ix.suspend()
        refused(lambda: ix.audit(), "suspended")
        assert L.ah_index_audit(ix._h, C.byref(rep), None) == 5 and rep.valid == 77
        ix.resume()
        f = ix.make_filter(dense.ids[::3])  # legal with a live filter
        assert ix.audit()["valid"] == 1
        f.close()
        assert L.ah_index_audit(ix._h, None, None) == 5 and b"out is NULL" in L.ah_last_error()
        raw = Dataset(DIST, DIMS, 10)
        try:
            raw.upload_vectors(np.arange(10, dtype=np.uint32), dense.vecs[:10])
            assert L.ah_forest_view_audit(raw._h, C.byref(view), C.byref(rep), None) == 7 and b"not finalized" in L.ah_last_error()
            assert rep.valid == 77
        finally:
            raw.close()
        big = _lib.AhForestView()
        C.memmove(C.byref(big), C.byref(view), C.sizeof(view))
        big.n_nodes = 1 << 32
        assert L.ah_forest_view_audit(dense.ds._h, C.byref(big), C.byref(rep), None) == 5 and b"32-bit" in L.ah_last_error()
        big.n_nodes, big.normal_stride = view.n_nodes, 8
        assert L.ah_forest_view_audit(dense.ds._h, C.byref(big), C.byref(rep), None) == 5 and b"stride" in L.ah_last_error()
        assert rep.valid == 77
    finally:
        ix.close()
