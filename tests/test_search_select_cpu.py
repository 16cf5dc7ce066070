"""The inputs of test_gpu_search_select.py, checked without a GPU: each designed input has the property it is named for —
its distances are the chosen words bit for bit, `selection` counts the 1024 or 1025 keys its name says, direct and scaled
spans and both edges of the k-th key's bin occur — and the oracle alone gives the answer numpy derives from the chosen
distances.  The reference stays within the condition: nothing here runs the code under test."""
import numpy as np
import pytest

import search_select_inputs as S
from oracle import oracle as O

CASES = S.capacity_cases()
METRIC = {"dot": O.DOT_PRODUCT, "euclid": O.EUCLIDEAN}


def oracle_of(case, sparse):
    od = O.Data(METRIC[case.metric], case.vectors, ids=case.ids(sparse) if sparse else None)
    if case.metric == "dot":
        od.preprocess_dot()
    return od


def oracle_answer(od, view, q, count, sk, cand=None):
    qv, qh = od.query_leaf(q)
    want, _ = O.search(od, None, qv, qh, count, sk, 0, cand, candidates_sorted=True, want_candidates=False, view=view)
    return np.array([i for i, _ in want], dtype=np.uint32), np.array([d for _, d in want], dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_words_round_trip_and_the_restated_bins():
    w = S.ordered_words(np.array([0.0, -0.0, 1.0, -1.0, np.inf, np.nan], dtype=np.float32))
    assert w[0] == w[1] == 0x80000000 and w[2] == S.W_ONE and w[3] < w[0] < w[2] < w[4] < w[5] == 0xFFFFFFFF
    some = np.array([S.W_ONE, S.W_ONE + 77, 0x7F000000, 0x80000001], dtype=np.uint64)
    assert S.ordered_words(S.f32_of_words(some)).tolist() == some.tolist()
    # the closed form of the largest word of a bin against a walk over the words, on spans around the ones the cases use
    for span in (2049, 4097, 2048 * 1024, S.span_with_bin_width(1025), 3_000_001):
        scale = (S.BINS << 32) // span
        for bin_k in (0, 1, 2, 1000, 2046, 2047):
            t = S.t_key_closed(0, span - 1, span, scale, bin_k)
            assert (t * scale) >> 32 <= bin_k and (t == span - 1 or ((t + 1) * scale) >> 32 > bin_k), (span, bin_k)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_case_has_the_property_it_is_named_for(case):
    od = oracle_of(case, False)
    for nq_i in (0, 3):
        q = case.queries(4)[nq_i]
        qv, qh = od.query_leaf(q)
        assert bits(od.distances(qv, qh)).tolist() == bits(case.distances(q)).tolist()  # the chosen words, bit for bit
        sel = S.selection(case.words(q), case.count)
        assert sel["n_sel"] == case.n_sel and sel["served"] == case.served, (case.name, sel)
        assert case.n_sel in (1024, 1025) or case.served
    for sparse in (False, True):
        ids = case.ids(sparse)
        assert (ids[-1] >= S.BITMAP_IDS) == sparse and np.array_equal(ids, np.arange(len(ids))) != sparse
        trees = case.trees(sparse)
        _v, ov, keep, listed = S.views(trees, METRIC[case.metric])
        assert listed <= 16384 and len(trees) == S.TREES
        assert np.array_equal(np.unique(np.concatenate(trees)), ids[case.listed])
        assert listed >= 7 * len(case.listed)  # every candidate in front of the de-duplication at least seven times
        od = oracle_of(case, sparse)
        cand = None if case.keep is None else ids[case.keep]
        for q in case.queries(4)[[0, 3]]:
            wi, wd = case.expect(q, sparse)
            gi, gd = oracle_answer(od, ov, q, case.count, listed, cand)
            assert gi.tolist() == wi.tolist() and bits(gd).tolist() == bits(wd).tolist(), case.name
            assert len(gi) == min(case.count, len(case.candidates()))


def test_the_cases_cover_both_kinds_of_span_both_bin_edges_and_both_outcomes():
    sels = {c.name: S.selection(c.words(c.queries(1)[0]), c.count) for c in CASES if c.n_sel}
    for metric in ("dot", "euclid"):
        mine = [sels[c.name] for c in CASES if c.metric == metric and c.n_sel]
        for direct in (True, False):
            assert {s["n_sel"] for s in mine if s["direct"] == direct} >= {1024, 1025}, (metric, direct)
    assert sels["ties-direct-1024"]["span"] == 2048 and sels["ties-span2049-1024"]["span"] == 2049
    last, first = sels["crowded-last-word-1024"], sels["crowded-first-word-1024"]
    assert not last["direct"] and last["kth"] == last["bin_last"] and last["bin_k"] == 0 and last["n_sel"] == 1024
    assert not first["direct"] and first["kth"] == first["bin_first"] and first["bin_k"] == 1 and first["n_sel"] == 1024
    over = sels["crowded-first-word-1025"]
    assert over["kth"] == over["bin_first"] and over["n_sel"] == 1025
    # equal distances around the k-th place: more keys on the k-th word than the selection is short of
    for name in ("ties-direct-1025", "ties-scaled-1025", "euclid-ties-1025", "euclid-equal-1025"):
        c = next(c for c in CASES if c.name == name)
        w = c.words(c.queries(1)[0])
        assert int((w == sels[name]["kth"]).sum()) >= 525 and int((w < sels[name]["kth"]).sum()) < c.count
    # distinct distances crowded into the k-th bin
    for name in ("crowded-1025", "crowded-first-word-1025", "same-ids-1025"):
        c = next(c for c in CASES if c.name == name)
        w = c.words(c.queries(1)[0])
        assert len(np.unique(w)) == len(w)
    assert any(c.count > len(c.candidates()) > 0 for c in CASES) and any(len(c.candidates()) == 0 for c in CASES)
    assert any(c.keep is not None and len(c.candidates()) == c.count for c in CASES)


def test_the_case_of_counts_beyond_the_capacity():
    case = S.big_count_case()
    q = case.queries(1)[0]
    w = case.words(q)
    assert len(np.unique(w)) == len(w) >= 2100
    for count in S.BIG_COUNTS:
        sel = S.selection(w, count)
        assert sel["served"] == (count <= S.CAP) and sel["n_sel"] >= count
    od = oracle_of(case, False)
    _v, ov, keep, listed = S.views(case.trees(False), METRIC[case.metric])
    for count in S.BIG_COUNTS:
        wi, wd = case.expect(q, False, count)
        gi, gd = oracle_answer(od, ov, q, count, listed)
        assert len(gi) == count and gi.tolist() == wi.tolist() and bits(gd).tolist() == bits(wd).tolist()


@pytest.mark.parametrize("metric", [O.COSINE, O.DOT_PRODUCT], ids=["cosine", "dot"])
@pytest.mark.parametrize("m", [1024, 1025])
def test_group_a_of_a_screened_case_is_the_answer_and_everything_else_is_far(metric, m):
    vecs, a, v = S.screened_case(m)
    od = O.Data(metric, vecs)
    if metric == O.DOT_PRODUCT:
        od.preprocess_dot()
    _v, ov, keep, listed = S.views(S.spread(np.arange(len(vecs), dtype=np.uint32)), metric)
    assert listed <= 16384
    for q in S.screened_queries(v, 4):
        qv, qh = od.query_leaf(q)
        d = od.distances(qv, qh)
        assert len(set(bits(d[a]).tolist())) == 1          # equal rows: equal distances, whatever the query
        rest = np.delete(d, a)
        if metric == O.COSINE:
            assert d[a[0]] < 0.005 and rest.min() > 0.99  # (the cosine distance is (1 - cos) / 2)
        else:
            assert d[a[0]] < -0.8 * float(v @ v) and rest.min() > 0.4 * float(v @ v)
        gi, gd = oracle_answer(od, ov, q, 1024, listed)
        assert gi.tolist() == a[:1024].tolist() and len(set(bits(gd).tolist())) == 1   # ties broken by id
