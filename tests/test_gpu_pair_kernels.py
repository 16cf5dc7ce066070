"""The row-major re-rank of a batched submission (`launch_inverted`, batch.hip): every kernel it can select.

A submission with >= 2 candidates per stored row is counting-sorted by row and its distances are computed row-major by one of

* k_pairs_distances_runs<M>       — AH_PAIR_RUNS != 0 and >= 3 pairs per stored row: the rows' runs of pairs, four per item;
* k_pairs_distances<M, 2 | 4 | 8> — otherwise: one pair per slot, AH_PAIR_GROUP pairs per octet (4 unless the tunable says 2 or 8).

Which kernel each (setting, mix) of this module selects:

    mix                          AH_PAIR_RUNS=1                      AH_PAIR_RUNS=0
    nq = 48, ~24 pairs per row   k_pairs_distances_runs (any group)  k_pairs_distances<M, AH_PAIR_GROUP>
    nq = 6,  2 - 3 pairs per row k_pairs_distances<M, AH_PAIR_GROUP> k_pairs_distances<M, AH_PAIR_GROUP>

so AH_PAIR_GROUP in {2, 8} is the only way to the <M, 2> and <M, 8> instantiations and AH_PAIR_RUNS=0 the only way to send a
list of >= 3 pairs per row to the pair-per-slot kernels.  AH_RERANK_INVERT=1 and AH_RERANK_SCREEN=0 keep the submission
row-major and unscreened.  dims 33: a scalar tail behind one 128-byte line; 70: three lines (an odd count); 128: four; 232:
a line pair plus the odd line (7.25).  Ids and distance bits must equal `Dataset.rerank` of every list, the oracle's `rerank`,
and one another across all six settings."""
import numpy as np
import pytest

import test_gpu_parity as P
from oracle import oracle as O
from test_gpu_parity import assert_bit_equal, make_data

pytestmark = pytest.mark.gpu

from arroy_amd import _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _imports():
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    P.D, P.O = D, O
    yield
    _lib.check(_lib.lib().ah_tuning_reset())


N, K = 1500, 25
ROW_MAJOR_METRICS = [0, 2, 3]  # `invert_legal`: f32 rows of >= 32 dims, not Manhattan
SETTINGS = [dict(AH_PAIR_GROUP=g, AH_PAIR_RUNS=r) for g in (2, 4, 8) for r in (0, 1)]


@pytest.mark.parametrize("nq", [48, 6])
@pytest.mark.parametrize("dims", [33, 70, 128, 232])
@pytest.mark.parametrize("metric", ROW_MAJOR_METRICS)
def test_every_row_major_pair_kernel_equals_single_reranks_and_the_oracle(metric, dims, nq):
    cls = D.BY_METRIC[metric]
    ds, oracle, _vecs, ids = make_data(cls, N, dims, seed=31 + 7 * metric + dims)
    rng = np.random.default_rng(9 + dims)
    qs = rng.standard_normal((nq, dims)).astype(np.float32)
    sizes = [int(x) for x in rng.integers(1, N, nq)] if nq > 6 else [N // 3] * nq
    sizes[0], sizes[1] = N, 0  # every row, and an empty list
    lists = [np.sort(rng.choice(ids, m, replace=False)).astype(np.uint32) for m in sizes]
    assert sum(sizes) >= 2 * N  # the library's policy threshold for the row-major path
    assert (sum(sizes) >= 3 * N) == (nq > 6)  # ... and for the row-run kernel
    # the references, once: Dataset.rerank and the oracle's rerank of every list
    want = []
    for i in range(nq):
        if sizes[i] == 0:
            want.append((np.zeros(0, np.uint32), np.zeros(0, np.float32)))
            continue
        ei, ed = ds.rerank(K, query=qs[i], sorted_ids=lists[i])
        q, qh = oracle.query_leaf(qs[i])
        ci, cd = oracle.rerank(q, qh, lists[i], K)  # (ids are row numbers here)
        assert list(ei) == [int(x) for x in ci], (metric, dims, nq, i)
        assert_bit_equal(ed, cd, f"single re-rank of list {i} vs the oracle")
        want.append((ei, ed))
    first = None
    scrub = np.ascontiguousarray(-qs[::-1])
    for knobs in SETTINGS:
        # The distances of a submission live in scratch that the next one reuses, pair for pair: a kernel that skipped a store
        # would find the previous setting's (equal) value in its place.  Other queries over the same lists in between leave
        # other values there.
        ds.rerank_batch(scrub, lists, K)
        with _lib.tuning(AH_RERANK_INVERT=1, AH_RERANK_SCREEN=0, **knobs):
            ds.rerank_stats(reset=True)
            oi, od, oc = ds.rerank_batch(qs, lists, K)
            st = ds.rerank_stats()
        assert st["queries_screened"] == 0, (knobs, st)
        for i in range(nq):
            ei, ed = want[i]
            assert int(oc[i]) == len(ei) and list(oi[i, : oc[i]]) == [int(x) for x in ei], (metric, dims, nq, knobs, i)
            assert_bit_equal(od[i, : oc[i]], ed, f"list {i} under {knobs}")
        if first is None:
            first = (oi.copy(), od.copy(), oc.copy())
        else:  # the padding behind the results included
            assert np.array_equal(oi, first[0]) and od.tobytes() == first[1].tobytes() and np.array_equal(oc, first[2]), knobs
    ds.close()
