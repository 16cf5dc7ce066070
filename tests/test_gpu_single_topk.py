"""The single-query top-k of ah_rerank_by_vector / ah_rerank_by_item (arroy_amd/csrc/distance.hip) where its three paths hand
over: the one-launch kernel (k_topk_small: n <= 16384, k <= 1024, finite distances, at most 1024 keys up to the k-th key's
bin, direct or scaled bins), the tournament (k_topk_round: buffers A / B) and the global bitonic sort (k > 2048, padded to
a power of two), and the skip of src/reader.rs:611-621, which the general path applies up to `skip_end`.

Every list runs twice through Dataset.rerank, with the defaults and with AH_RERANK_SMALL=0 (the general path alone), and
both answers are compared in full — ids as lists, distance bits with NaNs canonicalised — with two references, neither of
them the code under test: batch_topk_inputs.topk (numpy, rule="reference") and the oracle's statement-by-statement
median_based_top_k.  test_single_topk_cpu.py proves without a GPU which path each list takes, that the lists have the
properties they are named for, and that the two references agree on all of them.  A GPU test cannot see which kernel served
a list: that k_topk_small serves the lists meant for it rests on that CPU classification (single_path), and was checked once
by changing its `bin_of(w) <= bin_k` to `<`, which fails the limits, capacity and rounds tests here.

`late-admission` and `max-id-admitted` are the regression inputs of a defect this file found in the general path: it skipped
EVERY key >= (f32::MAX, u32::MAX) from position 2k on, lost a later +inf (or the item with id 0xFFFFFFFF) and returned a NaN
in its place; the reference stops skipping at the first key below that threshold.

Inputs: batch_topk_inputs.py (a Manhattan dataset of rows (c, 0, ..., 0) and a zero query: the distance of a row is |c|)."""
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

    def references(self, i, k, leaf=None, all_items=False):
        ei, ed = self.case.expect(i, k)
        wi, wd = self.oracle.rerank(*(leaf or self.leaf), None if all_items else self.case.rows[i], k)
        assert len(ei) == len(wi) == min(k, len(self.case.rows[i]))
        return (ei, ed), (wi, wd)

    def check(self, i, k, item=None, all_items=False):
        """List i at k through Dataset.rerank, with the defaults and on the general path: both equal both references."""
        what = (self.case.names[i], k, item, all_items)
        refs = self.references(i, k, None if item is None else self.oracle.item_leaf(int(np.flatnonzero(self.case.ids == item)[0])),
                               all_items)
        args = dict(sorted_ids=None if all_items else self.case.list_ids(i))
        args.update(dict(query=self.case.query) if item is None else dict(item=item))
        got = [self.ds.rerank(k, **args)]
        with _lib.tuning(AH_RERANK_SMALL=0):
            got.append(self.ds.rerank(k, **args))
        for path, (gi, gd) in zip(("default", "general"), got):
            for ref, (ri, rd) in zip(("numpy", "oracle"), refs):
                assert gi.tolist() == ri.tolist(), what + (path, ref)
                assert B.canonical_bits(gd).tolist() == B.canonical_bits(rd).tolist(), what + (path, ref)
        assert got[0][0].tolist() == got[1][0].tolist() and got[0][1].tobytes() == got[1][1].tobytes(), what
        return got[0]

    def close(self):
        self.ds.close()


@pytest.fixture(scope="module")
def distinct():
    staged = Staged(B.distinct_rows())
    yield staged
    staged.close()


@pytest.fixture(scope="module")
def nonfinite():
    """The non-finite lists at k = 8, 1100 and 2100, on a dataset with one more row, the all-zero one (for re-rank by item)."""
    staged = Staged(B.with_zero_row(B.nonfinite_case(B.SINGLE_NONFINITE_K)))
    yield staged
    staged.close()


def test_limits_of_the_one_launch_kernel(distinct):
    """n and k on both sides of topk_small_fits (16384, 1024), k = n, k > n, one item alone in a thread's last register slot,
    and the kernel's 1024 slots exactly full at n = 1025, 16383 and 16384."""
    st = distinct.with_lists(B.limits_case())
    for i, (n, k) in enumerate(B.LIMITS):
        ids, _ = st.check(i, k)
        assert len(ids) == min(n, k)


def test_capacity_with_direct_and_scaled_bins():
    """1024 selected keys (the one-launch kernel at its full width), 1025 (bit 3: the general path answers), exactly k, and
    the k-th key in bin 0 and in bin 2047 — over consecutive words, spans of 2048 (direct) and 2049 (scaled) words, +0 ... NaN
    (declined: bit 2) and +0 ... f32::MAX (scaled bins of 2^20 words, served by the kernel itself)."""
    st = Staged(B.capacity_case(B.CAP_K, B.SINGLE_SPREADS))
    for i in range(len(st.case)):
        st.check(i, B.CAP_K)
    st.close()


@pytest.mark.parametrize("k", B.SINGLE_TIES_K)
def test_ties_break_by_position(k):
    """9000 equal distances, and two values half and half: the order is the lists' (ascending ids, sparse and unequal to
    positions and rows), through the tournament (the one-launch kernel declines by bit 3) and, at 2049, the global sort."""
    st = Staged(B.ties_case())
    for i in range(2):
        ids, _ = st.check(i, k)
        if i == 0:
            assert ids.tolist() == st.case.list_ids(0)[:k].tolist()
    st.close()


@pytest.mark.parametrize("k", B.ROUNDS_K)
def test_tournament_rounds_and_final_buffers(distinct, k):
    """Lists of 1 to 5 rounds that end in buffer A and in buffer B, one call per list, the empty list included.  Up to 16384
    candidates and k <= 1024 it is the AH_RERANK_SMALL=0 run that reaches the tournament."""
    st = distinct.with_lists(B.rounds_case())
    for i, n in enumerate(B.ROUNDS_N):
        ids, _ = st.check(i, k)
        assert len(ids) == min(n, k)


@pytest.mark.parametrize("n", B.BITONIC_N)
def test_global_bitonic_sort_pads_with_sentinel_keys(distinct, n):
    """k > 2048 over lists that are and are not a power of two long; k = n returns the whole list in order (40 000 keys after
    padding to 65 536)."""
    st = distinct.with_lists(B.bitonic_case())
    i = B.BITONIC_N.index(n)
    for k in B.bitonic_ks(n):
        ids, dist = st.check(i, k)
        assert len(ids) == min(n, k)
        if k == n:
            assert sorted(ids.tolist()) == st.case.list_ids(i).tolist() and np.all(np.diff(dist) > 0)


@pytest.mark.parametrize("k", B.SINGLE_NONFINITE_K)
def test_non_finite_keys_and_the_skip_rule(nonfinite, k):
    """f32::MAX, +inf, NaN and the item with id 0xFFFFFFFF, before and after position 2k.  k = 8: k_topk_small raises bit 2
    and the tournament answers; k = 1100: the tournament; k = 2100: k_make_keys and the global sort."""
    picks = [i for i in range(len(nonfinite.case)) if nonfinite.case.names[i].startswith(f"{k}-")]
    assert len(picks) == 6
    for i in picks:
        nonfinite.check(i, k)


@pytest.mark.parametrize("k", B.SINGLE_NONFINITE_K)
def test_skipped_and_counted_keys_across_the_blocks_of_the_key_making_kernels(k):
    """Every block of k_topk_round<true> (4096 positions) and k_make_keys (256) finds skip_end for itself.  Lists of 14 000
    to 18 000: 9000 +inf / NaN after position 2k that are skipped over several blocks and many steps of the walk, the one
    finite key in a later block, and +inf / the item with id 0xFFFFFFFF that count in that block and in the blocks after
    it; then the longer list as "all items" of a dataset of its own (ids from the dataset's id array)."""
    case = B.far_case(k)
    st = Staged(case)
    for i in range(2):
        ids, dist = st.check(i, k)
        assert int(np.isinf(dist).sum()) == 4 and (B.MAX_ID in ids.tolist()) == (i == 1)
    st.close()
    st = Staged(B.own_dataset(case, 1))
    st.check(0, k, all_items=True)
    st.close()


def test_non_finite_keys_through_the_batch_calls_fallback(nonfinite):
    """ah_rerank_batch with k > 2048 queues the single-query kernels, one list after the other."""
    k, case = 2100, nonfinite.case
    picks = [i for i in range(len(case)) if case.names[i].startswith(f"{k}-")]
    qs = np.zeros((len(picks), B.DIMS), dtype=np.float32)
    oi, od, oc = nonfinite.ds.rerank_batch(qs, [case.list_ids(i) for i in picks], k)
    for j, i in enumerate(picks):
        m = min(k, len(case.rows[i]))
        assert int(oc[j]) == m, case.names[i]
        for ref, (ri, rd) in zip(("numpy", "oracle"), nonfinite.references(i, k)):
            assert oi[j, :m].tolist() == ri.tolist(), (case.names[i], ref)
            assert B.canonical_bits(od[j, :m]).tolist() == B.canonical_bits(rd).tolist(), (case.names[i], ref)
        assert np.all(oi[j, m:] == B.MAX_ID) and np.all(od[j, m:].view(np.uint32) == 0xFFFFFFFF), case.names[i]


@pytest.mark.parametrize("k", B.SINGLE_NONFINITE_K)
def test_all_items_of_a_dataset_with_sparse_ids(k):
    """Each max-id list as a dataset of its own, re-ranked without an id list: the keys' ids (the skip of the item with id
    0xFFFFFFFF) and the answer's ids come from the dataset's id array."""
    case = B.nonfinite_case(B.SINGLE_NONFINITE_K)
    for name in ("max-id-inside", "max-id-skipped", "max-id-admitted"):
        st = Staged(B.own_dataset(case, case.index(f"{k}-{name}")))
        st.check(0, k, all_items=True)
        st.close()


def test_all_items_of_a_dataset_with_identity_ids():
    """No id list and no id array: positions are rows are ids, on each of the three paths."""
    st = Staged(B.identity_case())
    for k in B.IDENTITY_K:
        st.check(0, k, all_items=True)
    st.close()


@pytest.mark.parametrize("k", B.SINGLE_NONFINITE_K)
def test_by_item(nonfinite, k):
    """ah_rerank_by_item with the all-zero row as the query: the same answers as by vector."""
    for name in ("late-admission", "mixed", "max-id-admitted"):
        nonfinite.check(nonfinite.case.index(f"{k}-{name}"), k, item=B.ZERO_ID)
