"""The int8 stages of the node-major screen for DotProduct (AH_SCREEN8_DOT=1; DESIGN.md §2.4, k_forest_screen_node_dot8): every
level node-major, the int8 copy kept whatever the data (AH_SCREEN8=1).  Dimensions: 32 = the AVX tier's minimum, one 128-byte int8
step; 40 = a tail that is no multiple of 32 and the zero-padded int8 tail; 768 = six steps, the widest rows of the pipelined
variant; 896 = past it, the variant without the pipeline."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

from arroy_amd import _lib  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

N, SPLIT_AFTER, SEEDS = 3000, 24, [11, 12, 13]


@pytest.mark.parametrize("kind", ["uniform", "norms", "special"])
@pytest.mark.parametrize("dims", [32, 40, 768, 896])
def test_dot_product_forest_with_the_int8_stages_equals_the_oracle(dims, kind):
    from arroy_amd import Dataset
    rng = np.random.default_rng(dims + len(kind))
    vecs = rng.uniform(-1, 1, (N, dims)).astype(np.float32)
    if kind == "norms":  # 1e-3 .. 1e3: after the preprocessing h0 e_x dominates the margins of the short rows
        vecs = (vecs * 10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
    if kind == "special":  # an all-zero row, a tiny one, one that holds an inf
        vecs[5], vecs[6], vecs[7, 3] = 0.0, np.float32(1e-30), np.inf
    ds = Dataset(D.DotProduct, dims, N)
    ds.upload_vectors(np.arange(N, dtype=np.uint32), vecs)
    ds.preprocess_dot()
    ds.finalize()
    oracle = O.Data(O.DOT_PRODUCT, vecs)
    oracle.preprocess_dot()

    def build(**tun):
        with _lib.tuning(AH_SCREEN8=1, **tun):
            f = ds.build_forest(SEEDS, split_after=SPLIT_AFTER, margin_mode=_lib.MARGIN_NODE_MAJOR)
        out = f.stats, f.digest()[0], [f.canonical(t) for t in range(len(SEEDS))]
        f.close()
        return out

    on, digest_on, trees_on = build(AH_SCREEN8_DOT=1)
    off, digest_off, _ = build(AH_SCREEN8_DOT=0)
    verified, digest_verified, _ = build(AH_SCREEN8_DOT=1, AH_SCREEN_VERIFY=1)
    ds.close()
    print(f"{kind} x {dims}: {on['screen8_decided']} + {on['screen8b_decided']} of {on['screen8_pairs']} pairs decided by stages 0 + 1")
    assert trees_on == [oracle.build_tree(SPLIT_AFTER, s).canonical() for s in SEEDS], "the forest differs from the oracle's"
    assert digest_on == digest_off == digest_verified
    assert off["screen8_pairs"] == 0  # the default: DotProduct without the int8 stages
    if kind != "special":
        assert on["screen8_pairs"] > 0 and on["screen8_decided"] > 0, on
    assert verified["screen_violations"] == 0 and verified["screen8_pairs"] == on["screen8_pairs"], verified
