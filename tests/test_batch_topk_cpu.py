"""The inputs of test_gpu_batch_topk.py, checked without a GPU: each designed input has the property it is named for, and
the two references the GPU answers are compared with — the oracle's restatement of median_based_top_k and the numpy one of
batch_topk_inputs.topk — agree on every one of them."""
import numpy as np
import pytest

import batch_topk_inputs as B
from oracle import oracle as O


def oracle_of(case):
    return O.Data(O.MANHATTAN, case.vectors, ids=case.ids)


agree = B.agree   # (the oracle against the numpy reference; shared with test_single_topk_cpu.py)


def test_the_distance_of_a_row_is_its_first_component_bit_for_bit():
    case = B.nonfinite_case()
    od = oracle_of(case)
    qv, qh = od.query_leaf(case.query)
    got = od.distances(qv, qh)
    assert B.canonical_bits(got).tolist() == B.canonical_bits(np.abs(case.c)).tolist()
    assert int(case.ids[-1]) == B.MAX_ID and case.c[-1] == B.F32_MAX
    assert np.all(np.diff(case.ids.astype(np.int64)) > 0) and not np.array_equal(case.ids, np.arange(len(case.ids)))


def test_ordered_words_and_rounds_restate_the_documented_design():
    w = B.ordered_words(np.array([0.0, -0.0, 1.0, B.F32_MAX, np.inf, np.nan, -np.nan, -1.0], dtype=np.float32))
    assert w[0] == w[1] == 0x80000000 and w[3] == B.MAX_WORD and w[4] == 0xFF800000 and w[5] == w[6] == 0xFFFFFFFF
    assert w[7] < w[0] < w[2] < w[3] < w[4] < w[5]
    assert [B.tour_rounds(n, min(n, 2048)) for n in (1, 4096, 4097, 8192, 8193)] == [1, 1, 2, 2, 3]
    assert B.tour_rounds(10 ** 6, 1) == 2 and B.tour_rounds(10 ** 6, 2048) > 5


def test_rounds_case_takes_one_to_five_rounds_and_ends_in_both_buffers():
    case = B.rounds_case()
    assert [len(r) for r in case.rows] == list(B.ROUNDS_N)
    assert len(np.unique(B.ordered_words(np.abs(case.c)))) == len(case.c) == 40000
    rounds = {n: B.tour_rounds(n, min(n, 2048)) for n in B.ROUNDS_N if n}
    assert rounds == {1: 1, 100: 1, 2047: 1, 2048: 1, 2049: 1, 4095: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3, 9000: 3,
                      20000: 4, 40000: 5}
    assert {B.final_buffer(n, min(n, 2048)) for n in rounds} == {"A", "B"}
    for k in (1025, 100, 1):  # the other k of the case: both buffers again, several round counts
        assert {B.final_buffer(n, min(n, k)) for n in rounds} == {"A", "B"}, k
    for i, n in enumerate(B.ROUNDS_N):
        if n == 0:
            continue
        for k in (100, 1):      # served by the selection ...
            assert case.select(i, k)["n_sel"] <= B.SEL_CAP, (n, k)
        for k in (2048, 1025):  # ... and left to the tournament exactly when more than 1024 keys are asked for
            assert case.select(i, k)["flagged"] == (min(n, k) > B.SEL_CAP), (n, k)
    agree(case, B.ROUNDS_K)


def test_capacity_case_sits_on_both_sides_of_the_selection_capacity():
    case = B.capacity_case()
    spans = {}
    for spread in B.SPREADS:
        sel = {name: case.select(case.index(f"{spread}-{name}"), B.CAP_K) for name in ("1024", "1025", "k", "bin0", "bin2047")}
        assert sel["1024"]["n_sel"] == 1024 and not sel["1024"]["flagged"], spread
        assert sel["1025"]["n_sel"] == 1025 and sel["1025"]["flagged"], spread
        assert sel["k"]["n_sel"] == B.CAP_K, spread
        assert sel["bin0"]["bin"] == 0 and not sel["bin0"]["flagged"], spread
        assert sel["bin2047"]["n_sel"] == 1010 and not sel["bin2047"]["flagged"], spread
        spans[spread] = sel["1024"]["span"]
        assert all(s["span"] == spans[spread] for n, s in sel.items() if n != "bin2047"), spread
        if spread in ("span2049", "wide"):  # scaled bins: the smallest word in bin 0, the largest in bin 2047
            assert not sel["1024"]["direct"] and sel["bin2047"]["bin"] == B.SEL_BINS - 1 and sel["bin2047"]["span"] == spans[spread]
        else:
            assert sel["1024"]["direct"]
    assert spans["consecutive"] == 21 and spans["span2048"] == 2048 and spans["span2049"] == 2049 and spans["wide"] >= 2 ** 31
    agree(case, (B.CAP_K,))


def test_ties_case_overflows_the_selection_at_every_k():
    case = B.ties_case()
    assert len(np.unique(case.dist(0))) == 1 and np.unique(case.dist(1), return_counts=True)[1].tolist() == [4500, 4500]
    for i in range(2):
        for k in B.TIES_K:
            assert case.select(i, k)["flagged"], (i, k)
            ids, _ = case.expect(i, k)
            assert np.all(np.diff(ids.astype(np.int64)) > 0)  # equal distances: by position, i.e. ascending ids
    assert B.tour_rounds(B.TIES_N, 1) == 2 and B.tour_rounds(B.TIES_N, 2048) == 3
    agree(case, B.TIES_K)


def test_nonfinite_case_is_decided_by_the_skip_rule():
    case = B.nonfinite_case()
    for k in B.NONFINITE_K:
        def differs(name, a, b):
            i = case.index(f"{k}-{name}")
            return case.expect(i, k, a)[0].tolist() != case.expect(i, k, b)[0].tolist()
        assert differs("skip-changes-answer", "reference", "none")
        assert not differs("skip-changes-answer", "reference", "every")
        assert differs("late-admission", "reference", "every") and differs("late-admission", "reference", "none")
        assert differs("max-id-skipped", "reference", "none") and differs("max-id-admitted", "reference", "every")
        assert not differs("mixed", "reference", "none") and not differs("mixed", "reference", "every")
        i = case.index(f"{k}-max-id-inside")
        assert len(case.rows[i]) <= 2 * k and B.MAX_ID in case.expect(i, k)[0].tolist()
        assert B.MAX_ID not in case.expect(case.index(f"{k}-max-id-skipped"), k)[0].tolist()
        assert B.MAX_ID in case.expect(case.index(f"{k}-max-id-admitted"), k)[0].tolist()
        for i in range(len(case)):
            if case.names[i].startswith(f"{k}-"):
                assert case.select(i, k)["flagged"] == (k > B.SEL_CAP), case.names[i]
    for k in B.NONFINITE_K:
        agree(case, (k,), [i for i in range(len(case)) if case.names[i].startswith(f"{k}-")])


def test_sub_batch_case_is_cut_after_1024_queries():
    case = B.sub_batch_case()
    n = [len(r) for r in case.rows]
    assert len(n) == B.SUB_QUERIES > 1024 and n[5] == 9000 and n[1027] == 20000
    assert all(n[q] == 0 for q in B.SUB_EMPTY) and all(3 <= x <= 40 for q, x in enumerate(n) if q not in B.SUB_BIG and q not in B.SUB_EMPTY)
    # the two parts differ in their key stride, and both long lists go to the tournament
    assert max(n[:1024]) == 9000 and max(n[1024:]) == 20000 and -(-9000 // B.CHUNK) != -(-20000 // B.CHUNK)
    assert case.select(5, B.SUB_K)["flagged"] and case.select(1027, B.SUB_K)["flagged"]
    agree(case, (B.SUB_K,))


def test_binary_quantized_case_classification():
    """BinaryQuantizedEuclidean distances are 4 * hamming: 65 possible values, so thousands of candidates tie.  Their f32
    words are far apart (scaled bins, not direct ones), and k = 1000 and 2048 overflow the selection while k = 5 does not."""
    vecs, queries = B.bq_case()
    od = O.Data(O.BQ_EUCLIDEAN, vecs)
    ids = np.arange(len(vecs), dtype=np.uint32)
    for q in queries:
        d = od.distances(*od.query_leaf(q))
        assert len(np.unique(d)) <= 65
        sel = {k: B.selection(d, ids, k) for k in B.BQ_K}
        assert not sel[5]["direct"] and not sel[5]["flagged"] and sel[1000]["flagged"] and sel[2048]["flagged"]


@pytest.mark.parametrize("k", [1, 2, 3, 7])
def test_numpy_reference_equals_the_oracle_on_random_non_finite_lists(k):
    """The statement of the skip in batch_topk_inputs.skipped against the oracle's statement-by-statement loop."""
    rng = np.random.default_rng(k)
    pool = np.array([0.0, 1.0, 2.0, 3.0, B.F32_MAX, np.inf, np.nan], dtype=np.float32)
    for _ in range(300):
        n = int(rng.integers(1, 6 * k + 4))
        d = pool[rng.choice(len(pool), n, p=[.05, .1, .1, .1, .15, .25, .25])]
        ids = np.sort(rng.choice(50, n, replace=False)).astype(np.uint32)
        if rng.random() < 0.5:
            ids[-1] = B.MAX_ID
        wi, wd = O.top_k(d, ids, min(k, n))
        ei, _ = B.topk(d, ids, k)
        assert wi.tolist() == ei.tolist(), (d.tolist(), ids.tolist())
