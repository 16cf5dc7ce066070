"""Shapes and rows of tests/test_gpu_dense_families.py, shared with the CPU check of its fallback cap
(tests/test_dense_families_cpu.py), so that both speak about the same rows, seeds and trees."""
import numpy as np

EUCLIDEAN, MANHATTAN, COSINE, DOT_PRODUCT = 0, 1, 2, 3
METRICS = [EUCLIDEAN, MANHATTAN, COSINE, DOT_PRODUCT]
METRIC_NAMES = {EUCLIDEAN: "euclidean", MANHATTAN: "manhattan", COSINE: "cosine", DOT_PRODUCT: "dot"}
# nk = round_up(dims, 64) / 64 = 1, 3, 5, 7, 10 k-blocks: one block (no second DMA), odd counts (the wide kernel's two-stage ring
# ends on stage 0), and a tail of one k-block after a steady trip of the narrow kernel's three-set ring (7, 10)
DIMS = [40, 160, 288, 416, 608]
N = 6001          # odd (k_forest_exact_pairs: unaligned side bytes), no multiple of 160 or 256 (a partial last row tile)
N_ALIGNED = 6400  # a multiple of 160, of 256 and of 4
ALIGNED_CASE = (EUCLIDEAN, 160)
TREES = 24
SPLIT_AFTER = 40
FALLBACK_CAP = 0.2  # share of the margin evaluations the screen may leave to the reference arithmetic (test_gpu_margin_modes.py)


def nk_of(dims):
    return (dims + 63) // 64


def data_seed(metric, dims, n):
    return 1000 * metric + dims + n


def tree_seeds(dims):
    return [int(x) for x in np.random.default_rng(dims + 5).integers(0, 2**63, TREES)]


def rows(n, dims, seed):
    """The rows `test_gpu_parity.make_data(cls, n, dims, seed)` uploads (unit scale): N(0, 1), two exact copies of row 1 and a
    zero row.  (The GPU test asserts that make_data really returned these.)"""
    vecs = np.random.default_rng(seed).standard_normal((n, dims)).astype(np.float32)
    vecs[3] = vecs[1]
    vecs[n // 2] = vecs[1]
    vecs[5] = 0.0
    return vecs


def dense_gamma_s(dims):
    """`da.gamma_s` of the dense MFMA screen (forest.hip): a chain of hpitch f32 roundings in any order, taken twice over."""
    hpitch = nk_of(dims) * 64
    return np.float32(2.0 * (hpitch + hpitch / 16 + 16.0) * 1.1920929e-7)


def splits_per_depth(trees):
    """Split nodes of the oracle's trees per depth: the columns of the build's levels.  `trees`: oracle.Tree objects."""
    counts = {}
    for tree in trees:
        for kind, _has_normal, _left, _right, _offset, _count, depth in tree.nodes:
            if kind == 2:
                counts[int(depth)] = counts.get(int(depth), 0) + 1
    assert sorted(counts) == list(range(len(counts))), counts
    return [counts[d] for d in range(len(counts))]
