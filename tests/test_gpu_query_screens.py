"""The certified top-k screens of ah_rerank_batch and ah_search_batch, checked against their own bounds.

Every case runs under AH_SCREEN_VERIFY=1: each candidate with a finite screen value is also evaluated in the reference's
f32 arithmetic and must lie in the interval [L, U] the selection derived for it (`Dataset.query_screen_verify`, counted by
k_screen_verify).  The answers are compared bit for bit with the oracle and with the same call with the screen off, and
the stats (`rerank_stats`, `Index.stats`) say which stage served the case, so that a fall-back cannot hide the path under
test.  Also: the ascending / unique contract of candidate lists on every path, and the window of the int8 stage's switch."""
import numpy as np
import pytest

from arroy_amd import Dataset, _lib, shard
from arroy_amd import distances as D
from oracle import oracle as O
from search_select_inputs import clustered  # (shared with test_gpu_search_select.py: one definition of the near-tie cluster)

pytestmark = pytest.mark.gpu

METRICS = [D.Cosine, D.DotProduct]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(cls, vecs):
    n, dims = vecs.shape
    ds = Dataset(cls, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    oracle = O.Data(cls.metric, vecs)
    if cls.metric == O.DOT_PRODUCT:
        ds.preprocess_dot()
        oracle.preprocess_dot()
    ds.finalize()
    return ds, oracle


def run(ds, qs, lists, k, **tun):
    """ah_rerank_batch under AH_SCREEN_VERIFY=1 and `tun`: (ids, distances, counts), rerank stats, verify counters."""
    with _lib.tuning(AH_SCREEN_VERIFY=1, **tun):
        ds.rerank_stats(reset=True)
        ds.query_screen_verify(reset=True)
        out = ds.rerank_batch(qs, lists, k)
        return out, ds.rerank_stats(), ds.query_screen_verify()


def same(a, b, what=""):
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y)), what


def canonical_nan(a):
    """Bits with every NaN as 0x7FC00000: the sign of the default NaN of an invalid operation is the platform's (x86, where
    the oracle runs, makes it negative; the GPU positive), so it differs between builds of the reference itself."""
    b = bits(a).copy()
    b[np.isnan(np.asarray(a, dtype=np.float32))] = 0x7FC00000
    return b


def check_oracle(oracle, qs, lists, k, out, picks, any_nan_sign=False):
    oi, od, oc = out
    view = canonical_nan if any_nan_sign else bits
    for i in picks:
        qv, qh = oracle.query_leaf(qs[i])
        wi, wd = oracle.rerank(qv, qh, np.asarray(lists[i], dtype=np.uint32), k)
        assert int(oc[i]) == len(wi), i
        assert oi[i, : oc[i]].tolist() == wi.tolist(), i
        assert view(od[i, : oc[i]]).tolist() == view(wd).tolist(), i


def three_ways(ds, oracle, qs, lists, k, picks=(0, 1, -1), expect_int8=True):
    """int8 first (the copy forced), binary16 only, unscreened: equal bits, the oracle's, counters proving each stage."""
    nq = sum(1 for l in lists if len(l))  # (an empty list has nothing to screen)
    a, st8, v8 = run(ds, qs, lists, k, AH_SCREEN8=1)
    assert v8["violations"] == 0 and v8["checked"] > 0, v8
    assert st8["queries_screened"] == nq and st8["chunks_int8_retried"] == 0, st8
    assert st8["chunks_int8"] == (1 if expect_int8 else 0), st8
    b, st16, v16 = run(ds, qs, lists, k, AH_RERANK_SCREEN8=0)
    assert v16["violations"] == 0 and v16["checked"] > 0, v16
    assert st16["queries_screened"] == nq and st16["chunks_int8"] == 0, st16
    c, st0, v0 = run(ds, qs, lists, k, AH_RERANK_SCREEN=0)
    assert st0["queries_screened"] == 0 and v0["checked"] == 0, (st0, v0)
    same(a, b, "int8 vs binary16")
    same(a, c, "screened vs unscreened")
    check_oracle(oracle, qs, lists, k, a, [p % nq for p in picks])
    with _lib.tuning(AH_SCREEN8=1):  # verify mode changes no answer
        same(a, ds.rerank_batch(qs, lists, k), "verify on vs off")
    return a, st8, st16


@pytest.mark.parametrize("cls", METRICS, ids=["cosine", "dot"])
@pytest.mark.parametrize("dims", [32, 96, 768, 1536])
def test_rerank_stages_hold_their_bounds(cls, dims):
    rng = np.random.default_rng(dims)
    n, nq, k = 3000, 12, 10
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    vecs[:, :3] *= np.float32(2.0 ** 10)   # columns whose scales differ by 2^20 (within binary16's range)
    vecs[:, 3:6] *= np.float32(2.0 ** -10)
    vecs[7] = 0.0
    ds, oracle = make(cls, vecs)
    qs = rng.standard_normal((nq, dims)).astype(np.float32)
    qs[1] = vecs[11]                           # a query equal to a row
    lists = [np.sort(rng.choice(n, 400, replace=False)).astype(np.uint32) for _ in range(nq)]
    lists[1] = np.union1d(lists[1], [7, 11]).astype(np.uint32)
    three_ways(ds, oracle, qs, lists, k)


def test_rerank_thresholds_of_the_screened_path():
    rng = np.random.default_rng(5)
    n, dims, nq = 9000, 64, 2
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    ds, oracle = make(D.Cosine, vecs)
    qs = rng.standard_normal((nq, dims)).astype(np.float32)

    def lists_of(total):
        per = [total // nq + (1 if i < total % nq else 0) for i in range(nq)]
        return [np.sort(rng.choice(n, m, replace=False)).astype(np.uint32) for m in per]

    for k, total, screened in ((256, 8 * 256 * nq, True), (257, 8 * 257 * nq, False), (256, 8 * 256 * nq - 1, False)):
        lists = lists_of(total)
        out, st, v = run(ds, qs, lists, k, AH_RERANK_SCREEN8=0)
        assert (st["queries_screened"] == nq) == screened, (k, total, st)
        assert v["violations"] == 0 and (v["checked"] > 0) == screened, (k, total, v)
        ref, _, _ = run(ds, qs, lists, k, AH_RERANK_SCREEN=0)
        same(out, ref, (k, total))
        check_oracle(oracle, qs, lists, k, out, [0, 1])
    # lists shorter than k, of length 1, and empty inside a screened submission
    k = 20
    lists = [np.sort(rng.choice(n, m, replace=False)).astype(np.uint32) for m in (4000, 5, 1, 0, 3000)]
    qs5 = rng.standard_normal((5, dims)).astype(np.float32)
    out, st, v = three_ways(ds, oracle, qs5, lists, k, picks=(0, 1, 2, 4))
    assert out[2].tolist() == [20, 5, 1, 0, 20]
    # >= 2 candidates per stored row: the row-major re-rank takes the submission, not the screen
    small_n = 300
    ds2, oracle2 = make(D.Cosine, vecs[:small_n].copy())
    lists = [np.arange(small_n, dtype=np.uint32)] * 3
    out, st, v = run(ds2, qs5[:3], lists, 10)
    assert st["queries_screened"] == 0 and v["checked"] == 0, (st, v)
    check_oracle(oracle2, qs5[:3], lists, 10, out, [0, 2])


@pytest.mark.parametrize("cls", METRICS, ids=["cosine", "dot"])
def test_near_ties_retry_on_binary16_then_the_exact_path(cls):
    rng = np.random.default_rng(17)
    dims, k = 256, 10
    # (the spread of the members' distances against the bounds: cosine ~0.044 s^2, dot ~16 s; int8 E ~50 x binary16 E)
    loose, tight = (0.15, 0.01) if cls is D.Cosine else (0.03, 0.001)
    # 3000 rows within the int8 error around the query: the int8 stage overflows, binary16 answers.  (DotProduct lists only
    # the members: distances of both signs, -256 and ~0, put the whole cluster into one bin of the selection's histogram.)
    vecs, centre = clustered(rng, 1000, 3000, dims, loose)
    ds, oracle = make(cls, vecs)
    lists = [np.arange(4000 if cls is D.Cosine else 3000, dtype=np.uint32)]
    qs = centre[None, :]
    out, st, v = run(ds, qs, lists, k, AH_SCREEN8=1)
    print("near ties, loose", cls.__name__, st["chunks_int8"], st["chunks_int8_retried"], st["queries_screened"], st["survivors"], v)
    assert st["chunks_int8_retried"] == 1 and st["queries_screened"] == 1, st
    assert v["violations"] == 0 and v["checked"] >= 2 * len(lists[0]), v  # both stages were verified
    ref, _, _ = run(ds, qs, lists, k, AH_RERANK_SCREEN=0)
    same(out, ref)
    check_oracle(oracle, qs, lists, k, out, [0])
    # a tighter cluster: binary16 overflows as well, the exact path answers
    vecs, centre = clustered(rng, 1000, 3000, dims, tight)
    ds, oracle = make(cls, vecs)
    qs = centre[None, :]
    out, st, v = run(ds, qs, lists, k, AH_SCREEN8=1)
    print("near ties, tight", cls.__name__, st["chunks_int8"], st["chunks_int8_retried"], st["queries_screened"], v)
    assert st["chunks_int8_retried"] == 1 and st["queries_screened"] == 0, st
    assert v["violations"] == 0 and v["checked"] >= 2 * len(lists[0]), v
    ref, _, _ = run(ds, qs, lists, k, AH_RERANK_SCREEN=0)
    same(out, ref)
    check_oracle(oracle, qs, lists, k, out, [0])


@pytest.mark.parametrize("cls", METRICS, ids=["cosine", "dot"])
def test_exact_duplicates_straddling_the_kth_place(cls):
    rng = np.random.default_rng(23)
    n, dims, k = 4000, 96, 10
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    q = rng.standard_normal(dims).astype(np.float32)
    vecs[100:130] = (q + vecs[100] * np.float32(0.01)).astype(np.float32)  # 30 copies of one row, the nearest by far
    ds, oracle = make(cls, vecs)
    lists = [np.arange(0, n, 2, dtype=np.uint32), np.arange(n, dtype=np.uint32)]
    qs = np.stack([q, q])
    out, _, _ = three_ways(ds, oracle, qs, lists, k, picks=(0, 1))
    assert out[0][1].tolist() == list(range(100, 110))  # ties broken by id


def special_case(ds, oracle, qs, lists, k, screened8, screened16, what, any_nan_sign=False):
    """Both screened stages against the unscreened path, single calls and the oracle; `screened*`: whether the stage must
    have answered the submission itself (None: not asserted)."""
    ref, _, _ = run(ds, qs, lists, k, AH_RERANK_SCREEN=0)
    for tun, want in (({"AH_SCREEN8": 1}, screened8), ({"AH_RERANK_SCREEN8": 0}, screened16)):
        out, st, v = run(ds, qs, lists, k, **tun)
        print("special", what, tun, st["queries_screened"], st["chunks_int8"], st["chunks_int8_retried"], v)
        assert v["violations"] == 0, (what, tun, v)
        if want is not None:
            assert (st["queries_screened"] == len(qs)) == want and (st["queries_screened"] == 0) == (not want), (what, tun, st)
        same(out, ref, (what, tun))
    check_oracle(oracle, qs, lists, k, ref, range(len(qs)), any_nan_sign)
    for i in range(len(qs)):
        ei, ed = ds.rerank(k, query=qs[i], sorted_ids=lists[i])
        assert ref[0][i, : ref[2][i]].tolist() == ei.tolist() and bits(ref[1][i, : ref[2][i]]).tolist() == bits(ed).tolist()


@pytest.mark.parametrize("cls", METRICS, ids=["cosine", "dot"])
def test_non_finite_and_degenerate_rows(cls):
    rng = np.random.default_rng(29)
    n, dims, k = 3000, 64, 10
    base_vecs = rng.standard_normal((n, dims)).astype(np.float32)
    base = np.sort(rng.choice(np.arange(100, n), 500, replace=False)).astype(np.uint32)
    # screenable: an all-zero row, rows in binary16's subnormal range, a row just above kTinyBits (2^-40), a zero query
    vecs = base_vecs.copy()
    vecs[30] = 0.0
    vecs[50] = (rng.standard_normal(dims) * 1e-11).astype(np.float32)
    vecs[60:62] = (rng.standard_normal((2, dims)) * 2e-5).astype(np.float32)
    ds, oracle = make(cls, vecs)
    qs = rng.standard_normal((4, dims)).astype(np.float32)
    qs[3] = 0.0
    lists = [np.union1d(base, r).astype(np.uint32) for r in ([30], [50], [60, 61], [30, 50, 60])]
    special_case(ds, oracle, qs, lists, k, True, True, "zero / subnormal / above tiny / zero query")
    # a row below kTinyBits: its norms cannot be measured.  int8: the row's scale is inf, a submission that lists it is not
    # screened; binary16: the dataset-wide maxima are inf, E is infinite and every candidate survives (501 of them: the
    # selection holds them, the survivors' f32 distances answer)
    vecs = base_vecs.copy()
    vecs[40] = (rng.standard_normal(dims) * 1e-13).astype(np.float32)
    ds, oracle = make(cls, vecs)
    special_case(ds, oracle, qs[:2], [np.union1d(base, [40]).astype(np.uint32)] * 2, k, False, True, "tiny row")
    # entries beyond 65504 (binary16 overflows: that stage never screens this dataset; the int8 copy scales the column),
    # an inf entry (not screened where listed), a query with an inf entry
    vecs = base_vecs.copy()
    vecs[10, 3] = np.float32(1e5)
    vecs[20, 5] = np.float32(np.inf)
    ds, oracle = make(cls, vecs)
    special_case(ds, oracle, qs[:2], [np.union1d(base, [10]).astype(np.uint32)] * 2, k, True, False, "entry beyond 65504")
    special_case(ds, oracle, qs[:2], [np.union1d(base, [20]).astype(np.uint32)] * 2, k, False, False, "inf entry")
    qi = qs[:2].copy()
    qi[1, 7] = np.float32(np.inf)
    special_case(ds, oracle, qi, [base, base], k, None, False, "query with an inf entry", any_nan_sign=True)


def test_long_lists_and_pipelined_groups():
    rng = np.random.default_rng(31)
    n, dims, k = 300_000, 32, 16
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    ds, oracle = make(D.Cosine, vecs)
    sizes = [100_000, 20_000, 17_000] + [13_000] * 32  # 553 k ids (> 512 Ki: the pipelined upload); one list beyond a group of 7
    qs = rng.standard_normal((len(sizes), dims)).astype(np.float32)
    lists = [np.sort(rng.choice(n, m, replace=False)).astype(np.uint32) for m in sizes]
    assert sum(sizes) >= 512 << 10 and sum(sizes) < 2 * n
    res = {}
    for g in (1, 2, 3, 7):
        out, st, v = run(ds, qs, lists, k, AH_RERANK_GROUPS=g, AH_SCREEN8=1)
        assert st["queries_screened"] == len(sizes) and v["violations"] == 0 and v["checked"] > 0, (g, st, v)
        res[g] = out
    for g in (2, 3, 7):
        same(res[1], res[g], g)
    ref, _, _ = run(ds, qs, lists, k, AH_RERANK_SCREEN=0)
    same(res[1], ref)
    check_oracle(oracle, qs, lists, k, res[1], [0, 1, 2, len(sizes) - 1])  # lists of 100 000, 20 000 and 17 000 (> 16 384)


def test_pipelined_groups_retry_and_fall_back():
    """A near-tie list inside a submission big enough for the pipelined upload (>= 512 Ki ids, in 3 groups): the int8 stage
    overflows and the binary16 rows answer (loose), or overflow as well and the exact path answers (tight) — the retry and
    the fall-back behind the groups, which no other test reaches.  List 0 and its rows are those of
    test_near_ties_retry_on_binary16_then_the_exact_path (same seed, same draws, same spreads 0.15 / 0.01); 266 000
    standard-normal rows and 53 lists of 10 000 of them follow.  (53, not 52: 4000 + 520 000 ids are fewer than 512 Ki =
    524 288, so the upload would not be pipelined; 534 000 are, and still fewer than 2 n = 540 000, where the row-major
    re-rank would take the submission.)  The spreads needed no change with the maxima of 270 000 rows; the commit before the
    two tails became one gave, with these inputs — loose: chunks_int8 0, chunks_int8_retried 1, queries_screened 54,
    survivors 901; tight: chunks_int8 0, chunks_int8_retried 1, queries_screened 0, survivors 0; 1 068 000 candidates
    checked against their intervals and no violation in either."""
    rng = np.random.default_rng(17)
    dims, k, n, n_far_lists = 256, 10, 270_000, 53
    near = [clustered(rng, 1000, 3000, dims, spread) for spread in (0.15, 0.01)]  # (loose, tight: the draws of that test)
    vecs = np.concatenate([near[0][0], rng.standard_normal((n - 4000, dims), dtype=np.float32)])
    lists = [np.arange(4000, dtype=np.uint32)]
    lists += [np.sort(rng.choice(np.arange(4000, n), 10_000, replace=False)).astype(np.uint32) for _ in range(n_far_lists)]
    qs = rng.standard_normal((len(lists), dims)).astype(np.float32)
    total = sum(len(l) for l in lists)
    assert 512 << 10 <= total < 2 * n
    for (rows, centre), screened in zip(near, (len(lists), 0)):
        vecs[:4000] = rows  # (only the cluster changes)
        qs[0] = centre
        ds, oracle = make(D.Cosine, vecs)
        out, st, v = run(ds, qs, lists, k, AH_RERANK_GROUPS=3, AH_SCREEN8=1)
        print("pipelined near ties", screened, st["chunks_int8"], st["chunks_int8_retried"], st["queries_screened"], st["survivors"], v)
        assert st["chunks_int8_retried"] == 1 and st["queries_screened"] == screened, st
        assert v["violations"] == 0, v
        one, _, _ = run(ds, qs, lists, k, AH_RERANK_GROUPS=1, AH_SCREEN8=1)
        same(out, one, "3 groups vs 1")
        ref, _, _ = run(ds, qs, lists, k, AH_RERANK_SCREEN=0)
        same(out, ref, "screened vs unscreened")
        check_oracle(oracle, qs, lists, k, out, [0, 1, len(lists) - 1])


@pytest.mark.parametrize("cls", METRICS, ids=["cosine", "dot"])
def test_unsorted_or_repeated_ids_are_rejected_on_every_path(cls):
    rng = np.random.default_rng(37)
    n, dims, k = 5000, 64, 10
    vecs = rng.standard_normal((n, dims)).astype(np.float32)
    ds, _ = make(cls, vecs)
    qs = rng.standard_normal((2, dims)).astype(np.float32)
    good = [np.sort(rng.choice(n, 1000, replace=False)).astype(np.uint32) for _ in range(2)]
    unsorted = [good[0], good[1].copy()]
    unsorted[1][[10, 500]] = unsorted[1][[500, 10]]
    repeated = [good[0], good[1].copy()]
    repeated[1][501] = repeated[1][500]
    for bad in (unsorted, repeated):
        with pytest.raises(_lib.ArroyHipError) as single:
            ds.rerank(k, query=qs[1], sorted_ids=bad[1])
        for tun in ({"AH_RERANK_SCREEN": 0}, {"AH_RERANK_SCREEN8": 0}, {"AH_SCREEN8": 1}):
            with _lib.tuning(**tun):
                ds.rerank_stats(reset=True)
                with pytest.raises(_lib.ArroyHipError) as batch:
                    ds.rerank_batch(qs, bad, k)
                assert batch.value.status == single.value.status, (tun, str(batch.value))
    # the pipelined path (>= 512 Ki ids in groups)
    big_n = 600_000
    ds2, _ = make(cls, rng.standard_normal((big_n, 32)).astype(np.float32))
    q2 = rng.standard_normal((4, 32)).astype(np.float32)
    lists = [np.sort(rng.choice(big_n, 140_000, replace=False)).astype(np.uint32) for _ in range(4)]
    lists[2] = lists[2].copy()
    lists[2][70_000] = lists[2][69_999]
    for tun in ({"AH_RERANK_GROUPS": 3, "AH_SCREEN8": 1}, {"AH_RERANK_GROUPS": 3, "AH_RERANK_SCREEN8": 0}, {"AH_RERANK_SCREEN": 0}):
        with _lib.tuning(**tun):
            with pytest.raises(_lib.ArroyHipError) as batch:
                ds2.rerank_batch(q2, lists, k)
            assert batch.value.status == single.value.status, (tun, str(batch.value))


def test_int8_switch_counts_overflows_in_windows_of_64():
    rng = np.random.default_rng(41)
    dims, k = 256, 10
    vecs, centre = clustered(rng, 1000, 3000, dims, 0.15)
    qn = rng.standard_normal((1, dims)).astype(np.float32)
    near = [np.arange(3000, dtype=np.uint32)]                                  # overflows the int8 stage
    far = [np.arange(3000, 4000, dtype=np.uint32)]
    with _lib.tuning(AH_SCREEN8=1):
        # 8 overflowing sub-batches, each followed by 15 good ones: at most 4 in any window of 64 — the stage stays on
        ds, _ = make(D.Cosine, vecs)
        ds.rerank_stats(reset=True)
        for _ in range(8):
            ds.rerank_batch(centre[None, :], near, k)
            for _ in range(15):
                ds.rerank_batch(qn, far, k)
        st = ds.rerank_stats()
        assert st["chunks_int8_retried"] == 8 and st["chunks_int8"] == 8 * 15, st
        ds.rerank_batch(qn, far, k)
        assert ds.rerank_stats()["chunks_int8"] == 8 * 15 + 1
        # 8 within 64: switched off
        ds, _ = make(D.Cosine, vecs)
        ds.rerank_stats(reset=True)
        for _ in range(8):
            ds.rerank_batch(centre[None, :], near, k)
            ds.rerank_batch(qn, far, k)
        st = ds.rerank_stats()
        assert st["chunks_int8_retried"] == 8 and st["chunks_int8"] == 7, st  # the 8th overflow switched it off
        ds.rerank_batch(qn, far, k)
        st = ds.rerank_stats()
        assert st["chunks_int8"] == 7 and st["queries_screened"] == 16 + 1, st


@pytest.fixture(scope="module")
def small_index():
    """100 k x 768 clustered rows (AH_SYNTH_CLUSTERED), 20 trees."""
    n, dims = 100_000, 768
    vecs = O.synth(7, 4, n, dims)
    ds = Dataset(D.Cosine, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32), vecs)
    ds.finalize()
    oracle = O.Data(O.COSINE, vecs)
    forest = ds.build_forest(shard.tree_seeds(42, range(20)))
    return ds, oracle, forest, ds.create_index(forest), vecs


def search_checked(index, ds, oracle, forest, count, sk, queries=None, items=None, picks=(0,), **tun):
    with _lib.tuning(AH_SCREEN_VERIFY=1, **tun):
        index.stats(reset=True)
        ds.query_screen_verify(reset=True)
        got = index.search(count, queries=queries, items=items, search_k=sk, raw=True)
        st, v = index.stats(), ds.query_screen_verify()
    assert v["violations"] == 0, (tun, v)
    with _lib.tuning(AH_SEARCH_SCREEN=0):
        plain = index.search(count, queries=queries, items=items, search_k=sk, raw=True)
    same(got, plain, tun)
    for i in picks:
        qv, qh = oracle.query_leaf(queries[i]) if queries is not None else oracle.item_leaf(int(items[i]))
        want, _ = O.search(oracle, forest, qv, qh, count, sk, want_candidates=False)
        assert got[0][i, : got[2][i]].tolist() == [a for a, _ in want], (tun, i)
        assert bits(got[1][i, : got[2][i]]).tolist() == bits(np.array([d for _, d in want], np.float32)).tolist(), (tun, i)
    return st, v


def test_search_int8_stage_on_a_small_index(small_index):
    ds, oracle, forest, index, vecs = small_index
    rng = np.random.default_rng(43)
    count, sk = 20, 2000
    for nq in (1, 8, 100):
        qs = (vecs[rng.choice(len(vecs), nq, replace=False)] + rng.standard_normal((nq, vecs.shape[1])) * 0.01).astype(np.float32)
        items = rng.choice(len(vecs), nq, replace=False).astype(np.uint32)
        for mv in (1, 4, 64):
            for by in ("vector", "item"):
                kw = {"queries": qs} if by == "vector" else {"items": items}
                st, v = search_checked(index, ds, oracle, forest, count, sk, picks=(0, nq - 1), AH_SEARCH_SCREEN8_MIN_QUERIES=1,
                                       AH_SEARCH_SCREEN8_MAX_VISITS=mv, AH_SCREEN8=1, **kw)
                assert st["rerank_screened"] + st["fallback_chunks"] * nq >= nq and v["checked"] > 0, (nq, mv, by, st, v)
                if nq > 1 and st["screen8_retried_chunks"] == 0:  # submissions past the small-submission kernels: int8 served
                    assert nq <= 64 or st["rerank_screened8"] == nq, (nq, mv, by, st)


def test_search_list_beyond_16384_candidates(small_index):
    ds, oracle, forest, index, vecs = small_index
    rng = np.random.default_rng(47)
    qs = (vecs[rng.choice(len(vecs), 4, replace=False)] + rng.standard_normal((4, vecs.shape[1])) * 0.01).astype(np.float32)
    st, v = search_checked(index, ds, oracle, forest, 30, 60_000, queries=qs, picks=(0, 3), AH_SEARCH_SCREEN8=0)
    assert st["rerank_screened"] == 4 and v["checked"] > 4 * 16_384, (st, v)
