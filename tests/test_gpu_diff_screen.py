"""The difference screen of ah_rerank_batch (AH_RERANK_SCREEN_DIFF=1): Euclidean / Manhattan lists scored on
the binary16 rows by k_pairs_screen_diff16, the survivors in f32.  Every call runs under AH_SCREEN_VERIFY=1; ids, distance bits
and counts are the oracle's and those of the same call at 0, and `rerank_diff_stats` says whether the stage answered,
overflowed or switched itself off.  The pruning cases' inputs and their share of survivors: test_diff_screen_bound_cpu.py."""
import numpy as np
import pytest

from arroy_amd import _lib
from arroy_amd import distances as D
from test_diff_screen_bound_cpu import pruning_inputs
from test_gpu_query_screens import check_oracle, make, same  # (the dataset with its oracle; equal bits; the oracle's re-rank)

pytestmark = pytest.mark.gpu
METRICS = pytest.mark.parametrize("cls", [D.Euclidean, D.Manhattan], ids=["euclidean", "manhattan"])
K = 10


def inputs(cls, case, dims):
    X, Q, lists = pruning_inputs("offset 100" if case == "offset 100" else "gaussian", dims)
    if case == "near-duplicates":  # 64 clusters of 64 rows, centres and members all closer together than delta (~2e-3)
        rng = np.random.default_rng(dims)
        centres = X[0] + rng.standard_normal((64, dims)).astype(np.float32) * np.float32(1e-4)
        X = (np.repeat(centres, 64, axis=0) + rng.standard_normal((4096, dims)) * 1e-5).astype(np.float32)
    if case == "non-finite":  # two candidates of the long list without a finite screen value
        X[lists[1][5], 0], X[lists[1][9], 1] = np.float32(1e6), np.float32(np.inf)
    return (*make(cls, X), Q, lists)


def run(ds, Q, lists, **tun):
    with _lib.tuning(AH_SCREEN_VERIFY=1, **tun):
        ds.rerank_stats(reset=True), ds.rerank_diff_stats(reset=True), ds.query_screen_verify(reset=True)
        out = ds.rerank_batch(Q, lists, K)
        return out, ds.rerank_stats(), ds.rerank_diff_stats(), ds.query_screen_verify()


@METRICS
@pytest.mark.parametrize("dims", [32, 72, 200])
@pytest.mark.parametrize("case", ["gaussian", "offset 100", "near-duplicates", "non-finite"])
def test_diff_screen_answers_like_the_f32_path(case, dims, cls):
    ds, oracle, Q, lists = inputs(cls, case, dims)
    nq, total = sum(1 for l in lists if len(l)), sum(len(l) for l in lists)  # (an empty list has nothing to screen)
    ref, st0, d0, v0 = run(ds, Q, lists, AH_RERANK_SCREEN_DIFF=0)
    assert st0["queries_screened"] == 0 and d0["chunks_screened"] == 0 and v0["checked"] == 0, (st0, d0, v0)
    out, st, d, v = run(ds, Q, lists, AH_RERANK_SCREEN_DIFF=1)
    print(case, dims, cls.__name__, d, v)
    same(out, ref), check_oracle(oracle, Q, lists, K, out, range(3))  # the call at 0 bit for bit, which is the oracle's
    assert v["violations"] == 0 and d["chunks_screened"] == 1 and d["switched_off"] == 0, (d, v)
    if case in ("gaussian", "offset 100"):
        assert v["checked"] > 0 and st["queries_screened"] == d["queries"] == nq, (st, d, v)
        assert K * nq <= st["survivors"] == d["survivors"] <= total // 2, (st, d)
    else:  # too many survivors, or a screen value that is not finite: the exact path answered
        assert st["queries_screened"] == d["queries"] == 0 and d["chunks_overflowed"] == (case == "near-duplicates"), (st, d)
    _, st, d, v = run(ds, Q, lists, AH_RERANK_SCREEN_DIFF=1, AH_RERANK_SCREEN=0)  # the older switch wins
    assert st["queries_screened"] == 0 and d["chunks_screened"] == 0 and v["checked"] == 0, (st, d, v)


@METRICS
def test_screened_from_eight_candidates_per_result(cls):
    ds, oracle, Q, _ = inputs(cls, "gaussian", 72)
    for sizes, screened in (((100, 140, 0), True), ((100, 139, 0), False)):  # 8 k nq = 240 candidates, and one short of it
        lists = [np.arange(5, 5 + m, dtype=np.uint32) for m in sizes]
        out, st, d, v = run(ds, Q, lists, AH_RERANK_SCREEN_DIFF=1)
        assert d["chunks_screened"] == screened and (v["checked"] > 0) == screened and v["violations"] == 0, (sizes, d, v)
        same(out, run(ds, Q, lists, AH_RERANK_SCREEN_DIFF=0)[0]), check_oracle(oracle, Q, lists, K, out, range(3))


def test_eight_overflows_switch_the_stage_off():
    ds, _, Q, lists = inputs(D.Euclidean, "near-duplicates", 32)
    ref = run(ds, Q, lists, AH_RERANK_SCREEN_DIFF=0)[0]
    with _lib.tuning(AH_RERANK_SCREEN_DIFF=1):
        for i in range(9):  # the ninth call finds the stage off
            same(ds.rerank_batch(Q, lists, K), ref)
            d = ds.rerank_diff_stats()
            assert (d["chunks_screened"], d["chunks_overflowed"], d["switched_off"]) == (min(i + 1, 8), min(i + 1, 8), i >= 7), (i, d)
