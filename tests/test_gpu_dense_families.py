"""Every kernel family of the dense MFMA screen of the build's top levels (dense_device.h; `dense_plan`, forest.hip), bit for bit
against the CPU oracle — the families only a tunable selects included.

`dense_plan` picks per level: k_forest_dense_narrow<M, 2> (160 x 64 tiles) up to 64 columns, k_forest_dense_narrow<M, 4>
(160 x 128 tiles, two epilogue rounds, groups of 12 row tiles once there is more than one column tile) up to
AH_DENSE_NARROW_MAX_COLS — 64 by default, so never without the switch —, k_forest_dense_screen<M, 2> (256 x 128) up to 128
columns and k_forest_dense_screen<M, 4> (256 x 256) beyond; AH_DENSE_NARROW_STREAM=1 selects the `STREAM = true` instantiations
of the narrow kernels, AH_DENSE_NARROW=0 sends levels 0 and 1 (one epilogue round spanning every tree) to the wide kernel.

Shapes (tests/dense_family_inputs.py): 24 trees over 6001 rows (odd; no multiple of a row tile) with split_after = 40 — levels of
24, 48, 96, ~192, ~384 ... columns, counted from the oracle's trees, never assumed — at dims 40, 160, 288, 416, 608: 1, 3, 5, 7
and 10 k-blocks of 64, i.e. a single block, odd counts for the wide kernel's two-stage ring, and every remainder of the narrow
kernel's ring of three register sets.  The screen's self-check is on (AH_SCREEN_VERIFY=1) and the share of the pairs it leaves to
the reference arithmetic is capped (tests/test_dense_families_cpu.py shows on the CPU that these rows sit far inside the cap), so
a kernel that decided nothing — the exact pass repairs everything — fails too."""
import numpy as np
import pytest

import dense_family_inputs as I
import test_gpu_parity as P
from oracle import oracle as O
from test_gpu_parity import check_forest_valid, make_data

pytestmark = pytest.mark.gpu

from arroy_amd import _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _imports():
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"
    P.D, P.O = D, O  # make_data / check_forest_valid live in test_gpu_parity and use its lazily imported modules
    yield
    _lib.check(_lib.lib().ah_tuning_reset())


NARROW_2, NARROW_4, WIDE_2, WIDE_4 = (160, 64), (160, 128), (256, 128), (256, 256)
# (e) is completed per case: AH_DENSE_MAX_COLS = the column count of level 2
SETTINGS = {"a": dict(), "b": dict(AH_DENSE_NARROW_MAX_COLS=256), "c": dict(AH_DENSE_NARROW_MAX_COLS=256, AH_DENSE_NARROW_STREAM=1),
            "d": dict(AH_DENSE_NARROW=0), "e": None}
CASES = [(m, d, I.N) for m in I.METRICS for d in I.DIMS] + [(*I.ALIGNED_CASE, I.N_ALIGNED)]


def expected_tiles(setting, cols):
    """The tile shape the issue's table promises for a level of `cols` columns under a setting."""
    if cols <= 64 and setting in "abce":
        return NARROW_2
    if 64 < cols <= 256 and setting in "bc":
        return NARROW_4
    if cols <= 128:  # (d) at any such level, (a) and (e) at 65 - 128 columns
        return WIDE_2
    return WIDE_4


@pytest.mark.parametrize("metric,dims,n", CASES, ids=[f"{I.METRIC_NAMES[m]}-{d}-{n}" for m, d, n in CASES])
def test_every_dense_family_builds_the_oracles_forest(metric, dims, n):
    cls = D.BY_METRIC[metric]
    ds, oracle, vecs, _ids = make_data(cls, n, dims, seed=I.data_seed(metric, dims, n))
    assert np.array_equal(vecs.view(np.uint32), I.rows(n, dims, I.data_seed(metric, dims, n)).view(np.uint32))  # the rows the CPU check saw
    seeds = I.tree_seeds(dims)
    trees = [oracle.build_tree(I.SPLIT_AFTER, s) for s in seeds]
    ref = [t.canonical() for t in trees]
    cols = I.splits_per_depth(trees)
    # the classes the families are chosen by all occur: <= 64 (levels 0, 1), 65 - 128, 129 - 256, several wide tiles
    assert cols[0] == I.TREES and cols[1] <= 64 and 64 < cols[2] <= 128 and 128 < cols[3] <= 256 and max(cols) > 512, cols
    assert I.nk_of(dims) in (1, 3, 5, 7, 10)
    digests, fallbacks = {}, {}
    for name, knobs in SETTINGS.items():
        knobs = dict(AH_DENSE_MAX_COLS=cols[2]) if knobs is None else knobs
        dense_levels = [c for c in cols if c <= knobs.get("AH_DENSE_MAX_COLS", 16384)]
        with _lib.tuning(AH_SCREEN_VERIFY=1, **knobs):
            forest = ds.build_forest(seeds, split_after=I.SPLIT_AFTER, margin_mode=_lib.MARGIN_DENSE_MFMA)
            shapes = {c: _lib.dense_tiles(n, c) for c in dense_levels}
            tiles_192 = _lib.launch_coverage(1, n, dims, cols[3]).shape if name == "b" else None
        what = f"{I.METRIC_NAMES[metric]} x {dims} (nk = {I.nk_of(dims)}), n = {n}, setting ({name}) {knobs}"
        st = forest.stats
        check_forest_valid(forest, n)
        for t in range(I.TREES):
            assert forest.canonical(t) == ref[t], f"tree {t} differs from the oracle: {what}"
        assert st["screen_violations"] == 0, (what, st)
        # the levels the setting makes dense, from the oracle's per-depth counts
        assert st["dense_launches"] == len(dense_levels) and st["dense_columns"] == sum(dense_levels), (what, st, cols)
        assert sum(st["margin_mode_launches"][1:7]) == 0, (what, st)
        if name == "e":  # the hand-over at the chosen level: 96 columns are dense, the ~192 of level 3 node-major
            assert len(dense_levels) < len(cols) and cols[3] not in dense_levels and st["margin_mode_launches"][0] > 0, (what, st, cols)
        # which kernel the plan of each dense level launches
        for c in dense_levels:
            assert shapes[c] == expected_tiles(name, c), (what, c, shapes[c])
        got = set(shapes.values())
        want = {"a": {NARROW_2, WIDE_2, WIDE_4}, "b": {NARROW_2, NARROW_4, WIDE_4}, "c": {NARROW_2, NARROW_4, WIDE_4},
                "d": {WIDE_2, WIDE_4}, "e": {NARROW_2, WIDE_2}}[name]
        assert got == want, (what, got)
        if name == "b":  # ~192 columns: two narrow column tiles of 128, the second one half padding
            assert tiles_192 == ((n + 159) // 160, 2) and cols[3] - 128 <= 64, (what, tiles_192, cols)
        digests[name] = forest.digest()[0]
        fallbacks[name] = (st["screen_fallbacks"], st["margin_evaluations"])
        forest.close()
    assert len(set(digests.values())) == 1, digests
    counts = ", ".join(f"({k}) {f} of {e}" for k, (f, e) in fallbacks.items())
    print(f"screen fallbacks, {I.METRIC_NAMES[metric]} x {dims}, n = {n}: {counts}")
    if metric != I.DOT_PRODUCT:
        for k, (f, e) in fallbacks.items():  # the screen decides the bulk of the pairs
            assert f < I.FALLBACK_CAP * e, f"setting ({k}): {counts}"
    else:
        # preprocessed DotProduct rows carry one huge extra dimension: the screen decides little, under any setting.  The
        # families differ only in the order of their f32 additions: near-equal counts, a factor 2 leaves room for that.
        for k in "bcd":
            assert fallbacks[k][0] < 2 * fallbacks["a"][0], f"setting ({k}): {counts}"
    ds.close()


@pytest.mark.parametrize("setting", ["a", "b", "d"])
def test_dense_block_maps_serve_every_tile_once_under_every_plan(setting):
    """k_dense_coverage runs `dense_block_map` with the plan `dense_plan` returns: 128-column narrow tiles and their grouping
    by 12 under (b), the wide map under (d), the mix of the default under (a)."""
    with _lib.tuning(**SETTINGS[setting]):
        for n, cols in [(6001, 96), (6001, 192), (1_000_003, 250), (10_000_000, 200)]:
            tiles = _lib.dense_tiles(n, cols)
            assert tiles == expected_tiles(setting, cols), (setting, n, cols, tiles)
            counts = _lib.launch_coverage(1, n, 768, cols)
            assert counts.shape == ((n + tiles[0] - 1) // tiles[0], (cols + tiles[1] - 1) // tiles[1])
            assert (counts == 1).all(), (setting, n, cols, int(counts.min()), int(counts.max()))
