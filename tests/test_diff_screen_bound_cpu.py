"""The difference screen of ah_rerank_batch (Euclidean / Manhattan, AH_RERANK_SCREEN_DIFF) restated in numpy
float32 on the copies and statistics of test_query_screen_bound_cpu.py: the kernel's f32 subtraction and accumulation
(search.hip: screen_diff8 / k_pairs_screen_diff16), screened_delta, screened_bounds_diff.  L <= d_ref <= U must hold against
the ORACLE's distances for every (query, row) pair with a finite screen value, whatever the order of the sum (no GPU)."""
import numpy as np
import pytest

from oracle import oracle as O
from test_query_screen_bound_cpu import F, case_data, gammas, lane_sums, query16, rows16

U24 = 5.9604645e-8
METRICS = pytest.mark.parametrize("metric", [O.EUCLIDEAN, O.MANHATTAN], ids=["euclidean", "manhattan"])
CASES = ["gaussian", "uniform", "offset 100", "near-duplicates", "column scales 2^+-10", "zero rows and query",
         "binary16 subnormal range", "tiny rows", "beyond 65504"]


def data_of(name, dims, rng):
    if name not in ("offset 100", "column scales 2^+-10"):
        return case_data(name, dims, rng)
    s, off = np.ones(dims, F), 100.0 if name == "offset 100" else 0.0  # (the common offset a dot-product bound could not serve)
    if not off:
        s[::3], s[1::3] = F(2.0 ** 10), F(2.0 ** -10)
    return ((off + rng.standard_normal((500, dims))) * s).astype(F), ((off + rng.standard_normal((5, dims))) * s).astype(F)


def bounds(metric, s, rmax, qs, dims):
    """screened_delta and screened_bounds_diff, with the factors screen_of_dataset sets."""
    one, euclid = F(1.0), metric == O.EUCLIDEAN
    g = F(F(2.0 * ((dims + 63) // 64 * 64 + 8.0) * U24) + F(1e-6))
    r = F((gammas(dims)[1] if euclid else F((dims + 2.0) * U24)) + F(1e-6))
    with np.errstate(invalid="ignore", over="ignore"):
        e2 = F(qs[1] + rmax[1])
        delta = F((e2 if euclid else F(np.sqrt(F(dims)) * e2)) * F(1.002) + F(1e-18))
        a = np.sqrt(s).astype(F) if euclid else s
        t_lo = np.fmax(F(0.0), (a * F(one - g) - delta).astype(F) * F(one - F(2e-7)))
        t_hi = (a * F(one + g) + delta).astype(F) * F(one + F(2e-7))
        p_lo, p_hi = ((t_lo * t_lo).astype(F), (t_hi * t_hi).astype(F)) if euclid else (t_lo, t_hi)
        return np.fmax(F(0.0), p_lo * F(one - r) - F(1e-37)).astype(F), (p_hi * F(one + r) + F(1e-37)).astype(F)


def intervals(metric, X, q):
    """{order: (L, U)}, {order: s} and d_ref of every row for one query.  d = q~ - x~ rounds once in f32; then an FMA chain of
    d^2 or a sum of |d|: in the lane order of the kernel, in sequence, reversed, and exactly."""
    data, dims = O.Data(metric, X), X.shape[1]
    (Xh, rmax), (qh, qs) = rows16(X), query16(q, dims)
    n, hp = len(X), (dims + 63) // 64 * 64
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.zeros((n, hp), F)
        d[:, :dims] = qh.astype(F)[None, :] - Xh.astype(F)
        term = d.astype(np.float64) ** 2 if metric == O.EUCLIDEAN else np.abs(d).astype(np.float64)  # (exact in f64)
        seq = lambda T: np.add.accumulate(T, axis=-1, dtype=F)[..., -1]  # noqa: E731
        # (lane_sums: lane j of the octet owns the pieces j, j + 8, ... of 8 elements, then the butterfly of octet_sum)
        s = {"lanes": lane_sums(term.astype(F), 8), "sequential": seq(term.astype(F)), "reversed": seq(term.astype(F)[:, ::-1]),
             "exact": term.sum(axis=1).astype(F)}
    return {o: bounds(metric, x, rmax, qs, dims) for o, x in s.items()}, s, data.distances(*data.query_leaf(q))


@METRICS
@pytest.mark.parametrize("dims", [32, 72, 200, 768])
@pytest.mark.parametrize("name", CASES)
def test_diff_screen_interval_holds(name, dims, metric):
    X, Q = data_of(name, dims, np.random.default_rng([dims, CASES.index(name)]))
    worst, checked = 0.0, 0
    for q in Q:
        lo_hi, s, d_ref = intervals(metric, X, q)
        for order, (lo, hi) in lo_hi.items():
            fin = (np.abs(s[order]) <= F(3.0e38)) & ~np.isnan(hi)  # (anything else: the selection takes the exact path)
            with np.errstate(invalid="ignore"):
                bad = fin & ~((lo <= d_ref) & (d_ref <= hi))
            assert not bad.any(), (name, dims, order, np.nonzero(bad)[0][:5], s[order][bad][:3], d_ref[bad][:3], lo[bad][:3], hi[bad][:3])
            checked += int(fin.sum())
            sel = fin & np.isfinite(hi) & (hi > lo)
            ratio = np.abs(s[order][sel].astype(np.float64) - d_ref[sel]) / ((hi[sel].astype(np.float64) - lo[sel]) / 2)
            worst = max([worst, *ratio.tolist()])
        if name == "beyond 65504":  # rows 3 (1e5) and 4 (inf) have no finite screen value, and delta is NaN: nothing is screened
            assert not np.isfinite(s["lanes"][3]) and not np.isfinite(s["lanes"][4]) and np.isnan(lo_hi["lanes"][1]).all()
    assert name in ("beyond 65504", "tiny rows") or checked > 0
    print(f"[diff bound] {name:26s} dims {dims:4d} {O.METRIC_NAMES[metric]:9s} max |s - d_ref| / half-width {worst:.3g}")


def pruning_inputs(case, dims):
    """Rows, queries and lists of test_gpu_diff_screen.py's pruning cases: 4096 rows, 3 queries, a list shorter than one tile of
    the screen kernel (512 candidates), one longer, an empty one."""
    rng = np.random.default_rng([7, dims])
    off = F(100.0 if case == "offset 100" else 0.0)
    X, Q = (off + rng.standard_normal((4096, dims))).astype(F), (off + rng.standard_normal((3, dims))).astype(F)
    return X, Q, [np.sort(rng.choice(4096, m, replace=False)).astype(np.uint32) for m in (300, 1500, 0)]


@METRICS
@pytest.mark.parametrize("dims", [32, 72, 200])
@pytest.mark.parametrize("case", ["gaussian", "offset 100"])
def test_pruning_inputs_leave_at_most_half_of_each_list(case, dims, metric, k=10):
    X, Q, lists = pruning_inputs(case, dims)
    for q, ids in zip(Q[:2], lists[:2]):
        lo, hi = intervals(metric, X, q)[0]["lanes"]
        survivors = int((lo[ids] <= np.sort(hi[ids])[k - 1]).sum())  # L <= T, T the k-th smallest U: the GPU test's cap
        assert k <= survivors <= len(ids) // 2, (case, dims, len(ids), survivors)
