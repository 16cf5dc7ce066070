"""Row-major levels of the three 1-bit metrics (AH_BUILD_ROWS_BQ=1; DESIGN.md §4 "1-bit row-major levels", k_forest_margin_rows_bq).
N = 3000 is no multiple of a slab (256 or 128 rows); five trees leave spare slots in a 16-slot and an 8-slot LDS group and make
tail_group_width cut a plain 16-slot schedule into 4 + 1.  Dimensions: 64 = one word, pitch 2; 70 = tail bits in the last word,
which must not count; 768 = 12 words (the 16-word rung); 2048 = 32 words, the widest rows the pass takes; 2112 = 33 words, which
stay node-major.  "special" rows at 768 dimensions: 200 copies of one row (failed splits, re-drawn normals and random sides behind
a row-major level), rows of 0.0 and -0.0 (sign bits 1 and 0), and rows whose margin against a root normal is exactly 0 (Right)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

from arroy_amd import _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

N, SPLIT_AFTER, SEEDS = 3000, 24, [11, 12, 13, 14, 15]
METRICS = pytest.mark.parametrize("cls", [D.BinaryQuantizedEuclidean, D.BinaryQuantizedManhattan, D.BinaryQuantizedCosine],
                                  ids=["bq-euclidean", "bq-manhattan", "bq-cosine"])
# margin_mode, and the margin_mode_launches entries its groups of five trees count in (ROWS_16: a 4-slot and a 2-slot group)
MODES = {"ROWS_2": (_lib.MARGIN_ROWS[2], (1,)), "ROWS_16": (_lib.MARGIN_ROWS[16], (1, 2)), "ROWS_LDS_8": (_lib.MARGIN_ROWS_LDS[8], (5,)),
         "ROWS_LDS_16": (_lib.MARGIN_ROWS_LDS[16], (6,)), "AUTO": (0, ())}


@functools.lru_cache(maxsize=None)
def reference(cls, dims, special=False):
    """The dataset, the oracle's trees and the digest and statistics of the node-major build (switch off), made once."""
    from arroy_amd import Dataset
    vecs = np.random.default_rng(dims).uniform(-1, 1, (N, dims)).astype(np.float32)
    if special:
        vecs[100:300] = vecs[100]
        vecs[5, 0::2], vecs[5, 1::2], vecs[6], vecs[7] = 0.0, -0.0, 0.0, -0.0
    ds = Dataset(cls, dims, N)
    ds.upload_vectors(np.arange(N, dtype=np.uint32), vecs)
    ds.finalize()
    oracle = O.Data(cls.metric, vecs)
    trees = [oracle.build_tree(SPLIT_AFTER, s) for s in SEEDS]
    if special:  # some row lies exactly on the root plane of some tree: margin = bias + 64 words - 2 hamming = +0.0
        rows = np.packbits(~np.signbit(vecs), axis=1, bitorder="little")
        zero = 0
        for t in trees:
            rec = np.frombuffer(t.normals, np.uint8)[t.nodes[t.root][4]:][: t.stride]
            ham = np.unpackbits(rows ^ rec[4:], axis=1).sum(axis=1)
            zero += int(np.sum(rec[:4].view(np.float32)[0] + np.float32(dims) - 2 * ham.astype(np.float32) == 0))
        assert zero > 0, "no row of the special data lies on a root plane"
    with _lib.tuning(AH_BUILD_ROWS_BQ=0):
        f = ds.build_forest(SEEDS, split_after=SPLIT_AFTER, margin_mode=_lib.MARGIN_ROWS[16])
    off = f.stats, f.digest()[0]
    f.close()
    return ds, [t.canonical() for t in trees], off


@METRICS
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dims,special", [(64, False), (70, False), (768, False), (2048, False), (768, True)],
                         ids=["64", "70", "768", "2048", "768-special"])
def test_row_major_1bit_levels_build_the_oracles_forest(cls, dims, special, mode):
    ds, want, (off, digest_off) = reference(cls, dims, special)
    margin_mode, counted = MODES[mode]
    with _lib.tuning(AH_BUILD_ROWS_BQ=1):
        f = ds.build_forest(SEEDS, split_after=SPLIT_AFTER, margin_mode=margin_mode)
    on, digest_on, trees = f.stats, f.digest()[0], [f.canonical(t) for t in range(len(SEEDS))]
    f.close()
    print(f"{mode} x {dims}: {on['margin_row_passes']} row passes, launches {on['margin_mode_launches']}")
    assert trees == want, "the forest differs from the oracle's"
    assert digest_on == digest_off
    assert off["margin_row_passes"] == 0 and sum(off["margin_mode_launches"][:7]) == 0, off  # switch off: node-major 1-bit only
    if counted:
        assert on["margin_row_passes"] > 0 and all(on["margin_mode_launches"][i] > 0 for i in counted), on


@METRICS
def test_rows_wider_than_32_words_stay_node_major(cls):
    ds, want, (off, digest_off) = reference(cls, 2112)
    with _lib.tuning(AH_BUILD_ROWS_BQ=1):
        f = ds.build_forest(SEEDS, split_after=SPLIT_AFTER, margin_mode=_lib.MARGIN_ROWS[16])
    on, digest_on, trees = f.stats, f.digest()[0], [f.canonical(t) for t in range(len(SEEDS))]
    f.close()
    assert trees == want and digest_on == digest_off
    assert on["margin_row_passes"] == 0 and on["margin_mode_launches"] == off["margin_mode_launches"], on


@METRICS
def test_the_encoded_stream_takes_the_row_major_levels_too(cls):
    ds, want, _ = reference(cls, 768)
    with _lib.tuning(AH_BUILD_ROWS_BQ=1):
        _roots, st, streamed = ds.build_forest_stream(SEEDS, split_after=SPLIT_AFTER, margin_mode=_lib.MARGIN_ROWS_LDS[16], encoded=True)
    assert [streamed.canonical(t) for t in range(len(SEEDS))] == want, "the streamed forest differs from the oracle's"
    assert st["margin_row_passes"] > 0 and st["margin_mode_launches"][6] > 0, st
