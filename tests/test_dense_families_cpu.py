"""The premise of the fallback cap of tests/test_gpu_dense_families.py, checked without a GPU.

That test builds forests with every level pinned to the dense MFMA screen and asserts that the screen leaves fewer than a fifth
of the margin evaluations to the reference arithmetic — otherwise a kernel that decided nothing would pass, the exact pass
repairing everything.  Here the same rows, seeds and trees go through the numpy restatement of the binary16 screen
(tests/test_screen_bound_cpu.py) with the dense product's gamma_s: for every split node of the oracle's trees, the pairs
(item under the node, the node's normal) the bound leaves undecided.  The share must sit well inside the cap, so that the
order of the matrix unit's additions (which the restatement does not know) cannot carry a correct kernel past it."""
import numpy as np
import pytest

import dense_family_inputs as I
from oracle import oracle as O
from test_screen_bound_cpu import stage_binary16

F = np.float32
N_TREES_CHECKED = 2  # of the 24: every tree draws its normals from the same rows, the share does not depend on the tree

CASES = [(m, d, I.N) for m in (I.EUCLIDEAN, I.MANHATTAN, I.COSINE) for d in I.DIMS] + [(*I.ALIGNED_CASE, I.N_ALIGNED)]


def undecided_and_evaluations(data, X, tree, metric, dims):
    """(pairs the dense screen's bound leaves open, margin evaluations) over the split nodes of one oracle tree."""
    hf = O.header_floats(metric)
    undecided = evaluations = 0

    def items_of(node):
        nonlocal undecided, evaluations
        kind, has_normal, left, right, offset, count, _depth = tree.nodes[node]
        if kind == 1:
            return np.asarray(tree.descendants[offset:offset + count], dtype=np.int64)
        items = np.concatenate([items_of(left), items_of(right)])
        if has_normal:
            rec = np.frombuffer(tree.normals[offset:offset + tree.stride], dtype=F)
            nv = rec[hf:hf + dims]
            bias = None if metric == I.COSINE else rec[0]
            s, e = stage_binary16(X[items], nv, dims, bias=bias, gamma_s=I.dense_gamma_s(dims))
            with np.errstate(invalid="ignore"):
                undecided += int((~(np.abs(s) > e)).sum())
            evaluations += items.size
        return items

    assert items_of(tree.root).size == len(X)
    return undecided, evaluations


@pytest.mark.parametrize("metric,dims,n", CASES, ids=[f"{I.METRIC_NAMES[m]}-{d}-{n}" for m, d, n in CASES])
def test_the_rows_of_the_dense_family_test_meet_its_fallback_cap(metric, dims, n):
    X = I.rows(n, dims, I.data_seed(metric, dims, n))
    data = O.Data(metric, X)
    undecided = evaluations = 0
    for seed in I.tree_seeds(dims)[:N_TREES_CHECKED]:
        tree = data.build_tree(I.SPLIT_AFTER, seed)
        u, e = undecided_and_evaluations(data, X, tree, metric, dims)
        assert e >= tree.margin_evals - tree.retries * n  # (a retried node evaluates its items once more)
        undecided += u
        evaluations += e
    share = undecided / evaluations
    print(f"{I.METRIC_NAMES[metric]} {dims} dims, n = {n}: {undecided} of {evaluations} pairs undecided ({share:.4f})")
    # a quarter of the cap: the GPU's accumulation order moves a screen value by less than gamma_s |n~||x~|, a small part of the bound
    assert share < I.FALLBACK_CAP / 4, (metric, dims, n, share)


def test_levels_of_the_dense_family_shapes():
    """The shapes were chosen so that the top levels have 24, 48, 96 and 192 columns and the ones below several hundred — one
    narrow tile, the 65-128 and 129-256 column classes and several wide tiles (level 4 has a few nodes fewer than 384: some
    children are leaves already).  The GPU test takes the counts from the oracle; this pins the premise."""
    for metric, dims in ((I.EUCLIDEAN, 40), (I.COSINE, 608)):
        X = I.rows(I.N, dims, I.data_seed(metric, dims, I.N))
        data = O.Data(metric, X)
        trees = [data.build_tree(I.SPLIT_AFTER, s) for s in I.tree_seeds(dims)]
        cols = I.splits_per_depth(trees)
        assert cols[:4] == [24, 48, 96, 192] and 256 < cols[4] <= 384, cols
        assert max(cols) > 512 and len(cols) >= 8, cols
