"""The encoded node stream on the device (arroy_amd/csrc/encode.hip): ah_encode_descendants and
ah_build_forest_stream_encoded hand out the bytes `NodeCodec` stores (src/node.rs:229-241).  References: what roaring-rs wrote
into tests/golden/large_v0_6.mdb, the plain restatement arroy_amd/node_codec.py, and the unencoded stream of the same seeds."""
import numpy as np
import pytest

import node_codec_cases as cases
from test_gpu_faults import DEVICE, OOM, sweep

pytestmark = pytest.mark.gpu

from arroy_amd import BuildCancelled, Dataset, _lib, node_codec  # noqa: E402
from arroy_amd import distances as D  # noqa: E402

INVALID_ARGUMENT = 5
BASE = 0x01020304


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import arroy_amd
    assert arroy_amd.device_count() >= 1, "no GPU visible: these tests must run on an MI355X"


def make(cls, n, dims, seed, ids=None, vecs=None):
    if vecs is None:
        vecs = np.random.default_rng(seed).standard_normal((n, dims)).astype(np.float32)
    ds = Dataset(cls, dims, n)
    ds.upload_vectors(np.arange(n, dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32), vecs)
    if cls.metric == 3:
        ds.preprocess_dot()
    ds.finalize()
    return ds


@pytest.fixture(scope="module")
def small():
    ds = make(D.Euclidean, 64, 32, seed=1)
    yield ds
    ds.close()


# ---- ah_encode_descendants ---------------------------------------------------------------------------------------------
def test_fixture_lists_encode_to_the_bytes_roaring_wrote(small):
    values = cases.fixture_descendants()
    assert len(values) == 59
    lists = [node_codec.decode_value(D.Euclidean, 30, v)[1] for v in values]
    assert small.encode_descendants(lists) == values


def test_edge_lists_and_a_scan_over_several_blocks(small):
    edge = cases.edge_lists()
    for name, ids in edge.items():  # one call each: a list alone, whatever its path
        assert small.encode_descendants([ids]) == [node_codec.encode_descendants(ids)], name
    together = list(edge.values())  # ... and in one call: bitmap lists between array lists
    assert small.encode_descendants(together) == [node_codec.encode_descendants(l) for l in together]
    rng = np.random.default_rng(9)
    many = [np.sort(rng.choice(1 << 20, size=int(k), replace=False)).astype(np.uint32) for k in rng.integers(0, 41, size=5000)]
    want = [node_codec.encode_descendants(l) for l in many]
    assert small.encode_descendants(many) == want  # 5000 lists: five tiles of the scan
    # out_values == NULL: the offsets alone
    ends = small.encode_descendants(many, sizes_only=True)
    assert ends.tolist() == np.concatenate(([0], np.cumsum([len(v) for v in want]))).tolist()
    assert small.encode_descendants([], sizes_only=True).tolist() == [0]


def test_unsorted_lists_and_a_short_cap_are_refused(small):
    good = np.array([1, 5, 70000], np.uint32)
    for bad in ([3, 3], [4, 3], [1, 2, 70000, 69999], list(range(100)) + [50]):
        with pytest.raises(_lib.ArroyHipError) as e:
            small.encode_descendants([good, np.array(bad, np.uint32), good])
        assert e.value.status == INVALID_ARGUMENT, bad
    need = int(small.encode_descendants([good, good], sizes_only=True)[2])
    with pytest.raises(_lib.ArroyHipError) as e:  # (Dataset.encode_descendants asserts that nothing lands past the values)
        small.encode_descendants([good, good], out_cap=need - 1)
    assert e.value.status == INVALID_ARGUMENT
    assert small.encode_descendants([good, good], out_cap=need) == [node_codec.encode_descendants(good)] * 2


# ---- the encoded stream against the unencoded one -------------------------------------------------------------------------
def check_encoded(ds, seeds, ref, ref_roots, base, **kw):
    roots, stats, got = ds.build_forest_stream(seeds, encoded=True, node_id_base=base, **kw)
    assert (roots.astype(np.int64) - base).tolist() == [int(r) for r in ref_roots]
    assert [got.canonical(t) for t in range(len(seeds))] == [ref.canonical(t) for t in range(len(seeds))]
    # same nodes in the same order with the same metadata
    assert list(got.splits) == list(ref.splits) and list(got.leaves) == list(ref.leaves)
    assert [v[1:] for v in got.splits.values()] == [v[1:] for v in ref.splits.values()]
    assert [v[1:] for v in got.leaves.values()] == [v[1:] for v in ref.leaves.values()]
    assert [(k, lvl) for k, lvl, _n, _b in got.batches if _n] and {b[0] for b in got.batches} == {1, 2}
    # every value is the restatement's encoding of the node it decodes to
    for nid, (nb, left, right, *_rest) in got.splits.items():
        assert got.values[nid] == node_codec.encode_split(left + base, right + base, nb), nid
    for nid, (ids, *_rest) in got.leaves.items():
        assert got.values[nid] == node_codec.encode_descendants(np.array(ids, np.uint32)), nid
    return stats, got


STREAM_CASES = [(D.Euclidean, 32, 3), (D.Cosine, 32, 3), (D.DotProduct, 32, 3), (D.BinaryQuantizedEuclidean, 32, 3),
                (D.Manhattan, 30, 3), (D.Cosine, 256, 2)]


@pytest.mark.parametrize("cls,dims,trees", STREAM_CASES, ids=[f"{c[0].__name__}-{c[1]}" for c in STREAM_CASES])
def test_encoded_stream_is_the_unencoded_stream_encoded(cls, dims, trees):
    """20 000 rows, split_after 8: thousands of leaves, empty ones included.  AH_READBACK_MB=1 (the smallest pinned double
    buffer: 1 MiB halves, node chunks of 4096) makes the Descendants of one build several chunks, and at 256 dimensions the
    split values of a level several pieces."""
    ds = make(cls, 20_000, dims, seed=dims + cls.metric)
    seeds = list(range(700, 700 + trees))
    with _lib.tuning(AH_READBACK_MB=1):
        for knobs, base in ((dict(AH_BUILD_TAIL_GROUPS=0), 0), (dict(AH_BUILD_TAIL_GROUPS=3, AH_BUILD_TAIL_MIN_MB=0, AH_ROWMAJOR=0), BASE)):
            with _lib.tuning(**knobs):
                ref_roots, ref_stats, ref = ds.build_forest_stream(seeds, split_after=8)
                stats, got = check_encoded(ds, seeds, ref, ref_roots, base, split_after=8)
            assert stats["tail_groups"] == ref_stats["tail_groups"] and stats["split_nodes"] == ref_stats["split_nodes"]
            assert knobs["AH_BUILD_TAIL_GROUPS"] == 0 or stats["tail_groups"] >= 2
            assert len(got.leaves) >= trees * 20_000 // 8  # thousands of leaves: several node chunks per Descendants job
            if dims == 256:  # values crossed pinned halves: more split batches than levels
                assert sum(1 for b in got.batches if b[0] == 2) > len({b[1] for b in got.batches if b[0] == 2})
    ds.close()


def test_leaves_with_bitmap_containers_inside_a_build():
    ds = make(D.Euclidean, 20_000, 32, seed=3)
    ref_roots, _stats, ref = ds.build_forest_stream([11, 12], split_after=6000)
    _stats, got = check_encoded(ds, [11, 12], ref, ref_roots, BASE, split_after=6000)
    assert max(len(leaf[0]) for leaf in got.leaves.values()) > 4096  # all ids below 65536: one bitmap container
    ds.close()


def test_one_node_trees_hold_bitmap_array_and_single_id_containers():
    ids = cases.edge_lists()["bitmap_array_one"]  # container 0: 4097 ids, container 1: 4096, container 9: one
    ds = make(D.BinaryQuantizedCosine, ids.size, 64, seed=4, ids=ids)
    for base in (0, BASE):
        roots, _stats, got = ds.build_forest_stream([1, 2], split_after=int(ids.size), encoded=True, node_id_base=base)
        assert roots.tolist() == [base, base + 1] and not got.splits
        assert [got.values[t] for t in (0, 1)] == [node_codec.encode_descendants(ids)] * 2
        assert [got.leaves[t][0] for t in (0, 1)] == [tuple(int(x) for x in ids)] * 2
    ds.close()


def test_identical_rows_give_nine_byte_split_values():
    vecs = np.tile(np.random.default_rng(8).standard_normal((1, 32)).astype(np.float32), (64, 1))
    ds = make(D.Euclidean, 64, 32, seed=0, vecs=vecs)
    ref_roots, _stats, ref = ds.build_forest_stream([5, 6], split_after=8)
    _stats, got = check_encoded(ds, [5, 6], ref, ref_roots, BASE, split_after=8)
    none = [nid for nid, s in got.splits.items() if s[0] is None]
    assert none and all(len(got.values[nid]) == 9 for nid in none)
    ds.close()


def test_base_overflow_and_a_stopping_sink_are_refused():
    ds = make(D.Euclidean, 5000, 32, seed=5)
    for base in (0xFFFFFFFF, 0xFFFFFFFF - 40):  # the roots alone pass 2^32 - 1; the first levels' children do
        with pytest.raises(_lib.ArroyHipError) as e:
            ds.build_forest_stream([1, 2, 3], split_after=20, encoded=True, node_id_base=base)
        assert e.value.status == INVALID_ARGUMENT, hex(base)
    calls = []

    def stop_at_third(batch):
        calls.append(int(batch.kind))
        return 7 if len(calls) == 3 else 0
    with pytest.raises(BuildCancelled):
        ds.build_forest_stream([1, 2, 3], sink=stop_at_third, split_after=20, encoded=True)
    assert len(calls) == 3
    ref_roots, _stats, ref = ds.build_forest_stream([1, 2, 3], split_after=20)  # and the dataset builds again afterwards
    check_encoded(ds, [1, 2, 3], ref, ref_roots, 0xFFFFFFFF - 8000, split_after=20)
    ds.close()


def test_stream_encoded_example_takes_the_same_values_from_both_sinks(tmp_path):
    """examples/stream_encoded.c at a small size: the host-encoding sink and the encoded stream fill their arenas with the
    same number of nodes and bytes and the same per-value checksum."""
    import re
    import subprocess
    from test_node_codec_cpu import build_stream_encoded_example
    exe = build_stream_encoded_example(tmp_path)
    seen = {}
    for mode in ("host", "encoded"):
        out = subprocess.run([exe, mode, "20000", "64", "4", "1"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        seen[mode] = re.findall(mode + r" build: .* s \(device .* s\), (\d+) nodes, (\d+) bytes, checksum (\d+)", out.stdout)
        assert len(seen[mode]) == 1 and f"{mode} median" in out.stdout, out.stdout
    assert seen["host"] == seen["encoded"] and int(seen["host"][0][1]) > 0, seen


def test_new_entry_points_survive_every_allocation_failure():
    ds = make(D.Cosine, 20_000, 64, seed=11)
    seeds = [101, 102, 103, 104]
    ref_roots, _stats, ref = ds.build_forest_stream(seeds)
    seen = sweep(lambda: ds.build_forest_stream(seeds, encoded=True, node_id_base=BASE))
    assert OOM in seen and all(s in (0, OOM, DEVICE) for s in seen), seen
    check_encoded(ds, seeds, ref, ref_roots, BASE)
    lists = list(cases.edge_lists().values())
    want = [node_codec.encode_descendants(l) for l in lists]
    seen = sweep(lambda: ds.encode_descendants(lists))
    assert len(seen) >= 7 and all(s in (OOM, DEVICE) for s in seen), seen
    assert ds.encode_descendants(lists) == want
    ds.close()
