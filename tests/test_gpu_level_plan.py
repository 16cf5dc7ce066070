"""What every level of a build chooses and launches (plan_level in arroy_amd/csrc/level_plan.h and the launchers of
BatchBuild::launch_level in forest.hip), pinned to the counts the build made before the plan was written down as one function.

Four shapes (those of test_gpu_margin_modes.py) x 16 / 13 / 7 trees x AUTO and seven forced modes, plus one build small enough
for the tail to run in groups of trees: the decision-bearing part of ah_build_stats and the forest's digest equal the values in
tests/golden/level_plan_stats.json, recorded with these same builds on commit 79a367ea478713016d145bbe7062038cd357a645.  They
are exact counts and hashes: no tolerance.  13 and 7 trees are where a wrong width of the last tree group shows (a launch
counted under another margin_mode_launches entry); the forced LDS modes at 1536 dimensions are where "does not fit" shows."""
import json
import os

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

from arroy_amd import _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

SHAPES = [("cosine768", D.Cosine, 768, 24_000), ("dot1536", D.DotProduct, 1536, 12_000), ("euclid128", D.Euclidean, 128, 30_000),
          ("manhattan256", D.Manhattan, 256, 20_000)]
TREES = (16, 13, 7)
MODES = (_lib.MARGIN_AUTO, 2, 4, 8, 16, 0x108, 0x110, 0x200)
FIELDS = ("dense_launches", "dense_columns", "margin_row_passes", "screened_launches", "rows_xcd_launches", "rows_nt_launches",
          "rows_split_launches", "margin_launches", "levels", "tail_groups")
GOLDEN = os.path.join(ROOT, "tests", "golden", "level_plan_stats.json")


def dataset(cls, dims, n, seed):
    from arroy_amd import Dataset
    ds = Dataset(cls, dims, n)
    ds.fill_synthetic(seed, 1, n)
    if cls is D.DotProduct:
        ds.preprocess_dot()
    ds.finalize()
    return ds


def decisions(forest):
    st = forest.stats
    out = {f: int(st[f]) for f in FIELDS}
    out["margin_mode_launches"] = [int(x) for x in st["margin_mode_launches"]]
    out["ah_forest_digest"] = f"{forest.digest()[0]:016x}"
    return out


def collect_shape(name):
    """{"<trees>/<mode>": decisions} of the 24 builds of one shape."""
    _, cls, dims, n = next(s for s in SHAPES if s[0] == name)
    ds = dataset(cls, dims, n, seed=dims)
    got = {}
    for trees in TREES:
        for mode in MODES:
            forest = ds.build_forest(list(range(700, 700 + trees)), margin_mode=mode)
            got[f"{trees}/{mode:#x}"] = decisions(forest)
            forest.close()
    ds.close()
    return got


def collect_tail():
    """A build small enough for the tail to run in groups (the knobs of test_gpu_tail_groups.py): where AUTO cuts it, and
    with every level node-major."""
    ds = dataset(D.Cosine, 96, 24_000, seed=96)
    got = {}
    for label, knobs in (("auto", {}), ("node_major", {"AH_ROWMAJOR": 0})):
        with _lib.tuning(AH_BUILD_TAIL_GROUPS=4, AH_BUILD_TAIL_MIN_MB=0, **knobs):
            forest = ds.build_forest(list(range(4100, 4109)))
        got[label] = decisions(forest)
        forest.close()
    ds.close()
    return got


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for key in want:
        assert got[key] == want[key], f"{what} {key}: {got[key]} != {want[key]}"


@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_every_level_chooses_and_launches_what_it_did(shape):
    want = recorded()[shape]
    assert len(want) == len(TREES) * len(MODES)
    assert_same(collect_shape(shape), want, shape)


def test_the_tail_is_cut_into_groups_where_it_was():
    want = recorded()["tail"]
    assert want["node_major"]["tail_groups"] == 4
    assert_same(collect_tail(), want, "tail")
