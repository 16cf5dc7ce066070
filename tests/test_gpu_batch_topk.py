"""The batched top-k of ah_rerank_batch (arroy_amd/csrc/batch.hip) where its two mechanisms hand over: the selection
(k_batch_topk_select: at most 1024 selected keys, direct or scaled bins, result written to the buffer the tournament would
have ended in), the tournament (k_batch_topk_round: per-query round counts inside one call, buffers A / B), the flag word
between them, the skip of src/reader.rs:611-621, the row-major distance path that borrows the key buffers first, and the cut
of a call into sub-batches of 1024 queries.

Every answer is compared — ids, distance bits and counts — with two references, neither of them the code under test: the
oracle's statement-by-statement median_based_top_k, and batch_topk_inputs.topk, a numpy sort of the chosen distance words.
test_batch_topk_cpu.py proves without a GPU that the inputs have the properties they are named for (rounds 1..5 with both
final buffers, 1024 / 1025 selected keys, spans of 2048 / 2049 words, the skip changing an answer) and that the two
references agree on all of them.

Inputs: batch_topk_inputs.py.  Non-finite distances come from non-finite row components: the upload accepts them, so no
detour over a non-finite query (as in test_gpu_small_calls.py) is needed.  Distances are compared through
`canonical_bits` (every NaN as 0x7FC00000, the view of test_gpu_query_screens.py): the sign and payload of a NaN that
arithmetic produced are the platform's.  (Manhattan's normalized distance is d.max(0.0), which turns a NaN distance into 0
on both sides; the NaNs that remain are the padding, which is checked to be exactly 0xFFFFFFFF.)

Out of scope: the cut of a sub-batch at 64 M candidate ids, which is too large for a test."""
import numpy as np
import pytest

import batch_topk_inputs as B
from arroy_amd import Dataset, _lib
from arroy_amd import distances as D
from oracle import oracle as O

pytestmark = pytest.mark.gpu


class Staged:
    """A case on the device and in the oracle."""

    def __init__(self, case):
        self.case = case
        self.ds = Dataset(D.Manhattan, B.DIMS, len(case.c))
        self.ds.upload_vectors(case.ids, case.vectors)
        self.ds.finalize()
        self.oracle = O.Data(O.MANHATTAN, case.vectors, ids=case.ids)
        self.leaf = self.oracle.query_leaf(case.query)

    def with_lists(self, case):
        other = Staged.__new__(Staged)
        other.case, other.ds, other.oracle, other.leaf = case, self.ds, self.oracle, self.leaf
        return other

    def run(self, picks, k):
        qs = np.zeros((len(picks), B.DIMS), dtype=np.float32)
        return self.ds.rerank_batch(qs, [self.case.list_ids(i) for i in picks], k)

    def check(self, picks, k, out, oracle_picks=None):
        oi, od, oc = out
        assert oi.shape == od.shape == (len(picks), k)
        for j, i in enumerate(picks):
            what = (self.case.names[i], k)
            ei, ed = self.case.expect(i, k)
            m = len(ei)
            assert int(oc[j]) == m == min(k, len(self.case.rows[i])), what
            assert oi[j, :m].tolist() == ei.tolist(), what
            assert B.canonical_bits(od[j, :m]).tolist() == B.canonical_bits(ed).tolist(), what
            assert np.all(oi[j, m:] == B.MAX_ID) and np.all(od[j, m:].view(np.uint32) == 0xFFFFFFFF), what
            if oracle_picks is None or i in oracle_picks:
                wi, wd = self.oracle.rerank(*self.leaf, self.case.rows[i], k)
                assert oi[j, :m].tolist() == wi.tolist(), what
                assert B.canonical_bits(od[j, :m]).tolist() == B.canonical_bits(wd).tolist(), what


def same_rows(a, ja, b, jb, what):
    for x, y in zip(a, b):
        assert np.array_equal(np.atleast_1d(x[ja]).view(np.uint32), np.atleast_1d(y[jb]).view(np.uint32)), what


@pytest.fixture(scope="module")
def distinct():
    staged = Staged(B.distinct_rows())
    yield staged
    staged.ds.close()


@pytest.mark.parametrize("k", B.ROUNDS_K)
def test_rounds_and_final_buffers_of_one_call(distinct, k):
    """k = 2048: lists of 1 to 5 rounds, ending in buffer A and in buffer B, in ONE call whose grid shrinks round by round;
    k = 1025: all but the shortest go to the tournament; k = 100 and 1: the selection serves every list, and writes into
    the buffer the list's own round count names.  The same lists reversed, and each in a call of its own (other strides,
    other `max_rounds`): the same rows."""
    st = distinct.with_lists(B.rounds_case())
    picks = list(range(len(st.case)))
    out = st.run(picks, k)
    st.check(picks, k, out)
    back = st.run(picks[::-1], k)
    for j, i in enumerate(picks):
        same_rows(out, j, back, len(picks) - 1 - j, (st.case.names[i], k, "reversed"))
        if len(st.case.rows[i]):  # (an empty call has no candidate array to pass)
            same_rows(out, j, st.run([i], k), 0, (st.case.names[i], k, "alone"))


def test_selection_capacity_with_direct_and_scaled_bins():
    """1024 selected keys (served by the selection at its full sort width), 1025 (flagged), exactly k, and the k-th key in
    bin 0 and in bin 2047 — over consecutive words, spans of 2048 (direct) and 2049 (scaled) words and +0 ... NaN."""
    st = Staged(B.capacity_case())
    picks = list(range(len(st.case)))
    st.check(picks, B.CAP_K, st.run(picks, B.CAP_K))
    st.check(picks[::-1], B.CAP_K, st.run(picks[::-1], B.CAP_K), oracle_picks=())
    st.ds.close()


@pytest.mark.parametrize("k", B.TIES_K)
def test_ties_break_by_position(k):
    """9000 equal distances, and two values half and half: the order is the lists' (ascending ids, sparse and unequal to
    positions and rows).  Every k overflows the selection."""
    st = Staged(B.ties_case())
    st.check([0, 1], k, st.run([0, 1], k))
    st.check([1, 0], k, st.run([1, 0], k), oracle_picks=())
    st.ds.close()


@pytest.mark.parametrize("k", B.NONFINITE_K)
def test_non_finite_keys_and_the_skip_rule(k):
    """f32::MAX, +inf, NaN and the item with id 0xFFFFFFFF, before and after position 2k; k = 8 through the selection and
    k = 1100 through the tournament.  `late-admission` and `max-id-admitted` are the regression inputs of a defect this
    file found: the skip used to be applied to EVERY key >= (f32::MAX, u32::MAX) from position 2k on, while the reference
    stops skipping at the first key below that threshold."""
    st = Staged(B.nonfinite_case())
    picks = [i for i in range(len(st.case)) if st.case.names[i].startswith(f"{k}-")]
    assert len(picks) == 6
    out = st.run(picks, k)
    st.check(picks, k, out)
    for j, i in enumerate(picks):
        same_rows(out, j, st.run([i], k), 0, (st.case.names[i], "alone"))
    st.ds.close()


def test_tournament_after_the_row_major_distances():
    """Euclidean lists that re-read rows take the row-major path, which keeps its pair lists in the key buffers before the
    selection writes its flag there: >= 3 pairs per row (row-run kernel) and 2.5 pairs per row (pair-per-slot kernel), k
    beyond the selection's capacity.  AH_RERANK_INVERT=0 (query-major distances): the same bits."""
    vecs, queries = B.euclid_case()
    n = len(vecs)
    ids = B.sparse_ids(n)
    ds = Dataset(D.Euclidean, B.DIMS, n)
    ds.upload_vectors(ids, vecs)
    ds.finalize()
    oracle = O.Data(O.EUCLIDEAN, vecs, ids=ids)
    rng = np.random.default_rng(9)
    all_rows = [np.arange(n, dtype=np.uint32) for _ in range(6)]
    some_rows = [np.sort(rng.choice(n, 2500, replace=False)).astype(np.uint32) for _ in range(3)]
    for rows, qs in ((all_rows, queries), (some_rows, queries[:3])):
        pairs = sum(len(r) for r in rows)
        assert (pairs >= 3 * n) if rows is all_rows else (2 * n <= pairs < 3 * n)
        lists = [ids[r] for r in rows]
        for k in (1500, 2048):
            out = ds.rerank_batch(qs, lists, k)
            with _lib.tuning(AH_RERANK_INVERT=0):
                plain = ds.rerank_batch(qs, lists, k)
            for j in range(len(rows)):
                same_rows(out, j, plain, j, (len(rows), k, j))
                wi, wd = oracle.rerank(*oracle.query_leaf(qs[j]), rows[j], k)
                assert int(out[2][j]) == len(wi) == k
                assert out[0][j].tolist() == wi.tolist() and out[1][j].tobytes() == wd.tobytes(), (len(rows), k, j)
    ds.close()


def test_sub_batches_of_a_call_of_1030_queries(distinct):
    """ah_rerank_batch cuts the call after 1024 queries; each part has its own key stride and round count (9000 candidates
    in query 5, 20 000 in query 1027).  Every row equals the same query in a call of its own."""
    st = distinct.with_lists(B.sub_batch_case())
    picks = list(range(len(st.case)))
    out = st.run(picks, B.SUB_K)
    st.check(picks, B.SUB_K, out, oracle_picks=B.SUB_PICKS)
    for i in picks:
        if len(st.case.rows[i]):
            same_rows(out, i, st.run([i], B.SUB_K), 0, (i, "alone"))


def test_binary_quantized_ties_from_real_kernel_output():
    """BinaryQuantizedEuclidean: 65 possible distances over 20 000 rows.  k = 5 is served by the selection, k = 1000 and 2048
    by the tournament (test_batch_topk_cpu.py classifies them)."""
    vecs, queries = B.bq_case()
    n = len(vecs)
    ds = Dataset(D.BinaryQuantizedEuclidean, vecs.shape[1], n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    ds.finalize()
    oracle = O.Data(O.BQ_EUCLIDEAN, vecs)
    rows = np.arange(n, dtype=np.uint32)
    for k in B.BQ_K:
        oi, od, oc = ds.rerank_batch(queries, [rows] * len(queries), k)
        for j, q in enumerate(queries):
            wi, wd = oracle.rerank(*oracle.query_leaf(q), rows, k)
            assert int(oc[j]) == len(wi) == k
            assert oi[j].tolist() == wi.tolist() and od[j].tobytes() == wd.tobytes(), (k, j)
    ds.close()
