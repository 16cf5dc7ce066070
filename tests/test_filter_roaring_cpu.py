"""ah_filter_create_roaring / ah_filter_create_roaring_batch without a GPU: the symbols against the header and the ctypes table,
arroy_amd/roaring.py (the restatement of the portable Roaring serialisation) against node_codec.encode_descendants and the
worked example of the header, and every refusal the library makes from the headers of the blobs alone — the structure of the
blobs is judged before the index is looked at, so with index = NULL a well-formed call ends in "index is NULL" and a malformed
one names its blob and container.  tests/test_gpu_filter_roaring.py imports the corpus."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from arroy_amd import node_codec, roaring
from conftest import ROOT

NEW_SYMBOLS = ("ah_filter_create_roaring", "ah_filter_create_roaring_batch")
EXAMPLE = bytes.fromhex("3B300100" "02" "0000020001000400" "010002000300" "010005000400")
EMPTY = bytes.fromhex("3A30000000000000")


def u32(a):
    return np.ascontiguousarray(sorted(set(int(x) for x in a)), dtype=np.uint32)


def corpus():
    """name -> ascending ids: every container kind, the kind thresholds, word edges, several keys."""
    rng = np.random.default_rng(11)
    span = 1 << 16
    sets = {
        "empty": [],
        "one_id": [5],
        "id_zero": [0],
        "array_4096": rng.choice(span, 4096, replace=False),
        "bitmap_4097": rng.choice(span, 4097, replace=False) + span,
        "bitmap_full": np.arange(span),
        "whole_span_run": np.arange(span, 2 * span),
        "word_edges": [0, 31, 32, 65535],
        "adjacent_words": list(range(20, 70)) + list(range(96, 128)) + [65535],
        "three_keys": [1, 2, 3] + list(range(span + 5, span + 10)) + [3 * span + 7],
        "four_keys": [1] + list(range(span, span + 300)) + [2 * span + 9, 5 * span],
        "nine_keys": [k * span + j for k in range(9) for j in range(k, 40 + k)],
        "dense_and_sparse": np.concatenate([np.arange(100, 9000), span + rng.choice(span, 50, replace=False), 2 * span + np.arange(0, span, 2)]),
        "last_id": [0xFFFFFFFF, 0xFFFF0000, 70000],
    }
    return {k: u32(v) for k, v in sets.items()}


def blobs_of(ids):
    """Both cookie forms, and under 12347 both states of the offset header the rule allows at this container count."""
    return [roaring.serialize(ids), roaring.serialize(ids, runs=True)]


def test_new_symbols_are_declared_exported_and_bound():
    from arroy_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "arroy_hip.h")).read()
    declared = set(re.findall(r"^AH_API [^;(]*?\b(ah_[a-z_0-9]+)\s*\(", header, re.M))
    assert "global: ah_*;" in open(os.path.join(ROOT, "arroy_amd", "csrc", "exports.map")).read()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.ah_abi_version() == 7
    assert C.sizeof(_lib.AhFilterRoaringStats) == 9 * 8
    assert C.sizeof(_lib.AhFilterStats) == 8 * 8  # the layouts existing callers pass have not grown
    m = re.search(r"typedef struct ah_filter_roaring_stats \{(.*?)\} ah_filter_roaring_stats;", header, re.S)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f for f, _ in _lib.AhFilterRoaringStats._fields_]


def test_serialize_and_deserialize_round_trip_and_equal_the_node_codec():
    rng = np.random.default_rng(1)
    sets = list(corpus().values())
    for _ in range(20):
        n = int(rng.integers(1, 9000))
        hi = int(rng.choice([100, 1 << 16, 1 << 18, 1 << 32]))
        sets.append(u32(rng.integers(0, hi, n, dtype=np.uint64)))
        start = int(rng.integers(0, 1 << 20))
        sets.append(u32(range(start, start + n)))
    for ids in sets:
        plain = roaring.serialize(ids)
        assert plain == node_codec.encode_descendants(ids)[1:]  # (pinned to the reference's bytes by the node codec's tests)
        assert np.array_equal(roaring.deserialize(plain), ids)
        nc = len(roaring.containers(ids))
        for off in (None, True, False):
            if nc == 0 or (off is not None and off != (nc >= roaring.NO_OFFSET_THRESHOLD)):
                continue
            packed = roaring.serialize(ids, runs=True, offsets=off)
            assert np.array_equal(roaring.deserialize(packed), ids) and len(packed) <= len(plain) + (nc + 7) // 8
        got = node_codec.decode_value(None, 0, bytes([node_codec.TAG_DESCENDANTS]) + plain)
        assert got[0] == "D" and np.array_equal(got[1], ids)


def test_the_worked_example_and_the_empty_bitmap_byte_for_byte():
    ids = u32([1, 2, 3] + list(range(65541, 65546)))
    assert roaring.serialize(ids, runs=True) == EXAMPLE and len(EXAMPLE) == 25
    assert np.array_equal(roaring.deserialize(EXAMPLE), ids)
    assert roaring.serialize([]) == roaring.serialize([], runs=True) == EMPTY and roaring.deserialize(EMPTY).size == 0
    assert roaring.kinds(EXAMPLE) == {0: roaring.ARRAY, 1: roaring.RUN}
    # run-encoding only where it is smaller: a run of the whole span is 6 bytes, three scattered ids stay an array
    assert roaring.kinds(roaring.serialize(np.arange(1 << 16, dtype=np.uint32), runs=True)) == {0: roaring.RUN}
    assert roaring.kinds(roaring.serialize(u32([1, 5, 9]), runs=True)) == {0: roaring.ARRAY}
    # the offset header under 12347: from four containers on
    for nc, want in ((3, False), (4, True)):
        ids = u32(k << 16 for k in range(nc))
        assert len(roaring.serialize(ids, runs=True)) == 4 + 1 + 4 * nc + (4 * nc if want else 0) + 2 * nc


# ---- refusals from the headers alone ------------------------------------------------------------------------------------------

def call_batch(L, blobs, out=True):
    arrs = [np.frombuffer(b, dtype=np.uint8) if b is not None else None for b in blobs]
    n = len(arrs)
    ptrs = (C.c_void_p * max(1, n))(*[a.ctypes.data if a is not None else None for a in arrs])
    lens = (C.c_size_t * max(1, n))(*[a.size if a is not None else 0 for a in arrs])
    handles = (C.c_void_p * max(1, n))(*([0xDEAD] * max(1, n)))
    status = L.ah_filter_create_roaring_batch(None, ptrs, lens, n, handles if out else None, None)
    if out:
        assert all(handles[i] is None for i in range(n)), "every out[i] is NULL after a refusal"
    return status, L.ah_last_error().decode()


def malformations():
    """name -> (blob, the container the refusal names or None, a word of the refusal)"""
    good = roaring.serialize(corpus()["four_keys"], runs=True)  # 12347, four containers: flags, offsets, a run container
    plain = roaring.serialize(corpus()["three_keys"])
    assert roaring.kinds(good)[1] == roaring.RUN
    out = {}
    out["truncated_cookie"] = (good[:3], None, "shorter")
    out["truncated_header_12347"] = (good[:4 + 1 + 16 + 7], None, "shorter than the headers")
    out["truncated_header_12346"] = (plain[:8 + 12 + 11], None, "shorter than the headers")
    out["bad_cookie"] = (struct.pack("<I", 12345) + good[4:], None, "unknown cookie")
    keys = bytearray(good)
    keys[5 + 8:5 + 10] = struct.pack("<H", 1)  # container 2's key: 1 after 1
    out["keys_not_ascending"] = (bytes(keys), 2, "ascend")
    desc = bytearray(plain)
    desc[8 + 4:8 + 6] = struct.pack("<H", 0)  # container 1's key: 0 after 0
    out["keys_descending_12346"] = (bytes(desc), 1, "ascend")
    out["payload_past_len"] = (good[:-1], 3, "past")
    card = bytearray(plain)
    card[8 + 2:8 + 4] = struct.pack("<H", 4000)  # container 0 claims 4001 values: its array ends behind the blob
    out["cardinality_past_len"] = (bytes(card), 0, "past")
    off = bytearray(good)
    at = 5 + 16 + 4 * 2
    off[at:at + 4] = struct.pack("<I", struct.unpack_from("<I", good, at)[0] + 2)
    out["wrong_offset"] = (bytes(off), 2, "offset entry")
    out["trailing_bytes"] = (good + b"\0", None, "the containers end at")
    out["trailing_bytes_12346"] = (plain + b"\0\0", None, "the containers end at")
    runs = bytearray(good)
    (run_at,) = struct.unpack_from("<I", good, 5 + 16 + 4)
    runs[run_at:run_at + 2] = struct.pack("<H", 500)  # container 1 claims 500 runs
    out["run_count_past_len"] = (bytes(runs), 1, "past")
    return out


def test_well_formed_blobs_reach_the_index_check():
    from arroy_amd import _lib
    L = _lib.lib()
    every = [b for ids in corpus().values() for b in blobs_of(ids)] + [EXAMPLE, EMPTY]
    for b in every:
        h = C.c_void_p(0xDEAD)
        a = np.frombuffer(b, dtype=np.uint8)
        assert L.ah_filter_create_roaring(None, a.ctypes.data, a.size, C.byref(h)) == 5 and h.value is None
        assert "index is NULL" in L.ah_last_error().decode(), (b[:16], L.ah_last_error())
    status, text = call_batch(L, every)
    assert status == 5 and "index is NULL" in text, text
    # a copy at an odd address parses the same
    buf = np.zeros(len(EXAMPLE) + 1, dtype=np.uint8)
    buf[1:] = np.frombuffer(EXAMPLE, dtype=np.uint8)
    h = C.c_void_p()
    assert L.ah_filter_create_roaring(None, buf.ctypes.data + 1, len(EXAMPLE), C.byref(h)) == 5 and "index is NULL" in L.ah_last_error().decode()
    # n == 0: AH_OK, nothing looked at
    st = _lib.AhFilterRoaringStats()
    out = (C.c_void_p * 1)()
    assert L.ah_filter_create_roaring_batch(None, None, None, 0, out, C.byref(st)) == 0 and st.filters == 0


def test_argument_refusals_come_first_and_in_order():
    from arroy_amd import _lib
    L = _lib.lib()
    bad = malformations()["bad_cookie"][0]
    status, text = call_batch(L, [bad, None, EMPTY], out=False)
    assert status == 5 and "out is NULL" in text
    h = C.c_void_p(0xDEAD)
    assert L.ah_filter_create_roaring(None, None, 0, None) == 5 and "out is NULL" in L.ah_last_error().decode()
    assert L.ah_filter_create_roaring(None, None, 0, C.byref(h)) == 5 and "blobs[0] is NULL" in L.ah_last_error().decode() and h.value is None
    out = (C.c_void_p * 3)()
    lens = (C.c_size_t * 3)(8, 8, 8)
    ptrs = (C.c_void_p * 3)()
    assert L.ah_filter_create_roaring_batch(None, None, lens, 3, out, None) == 5 and "blobs is NULL" in L.ah_last_error().decode()
    assert L.ah_filter_create_roaring_batch(None, ptrs, None, 3, out, None) == 5 and "lens is NULL" in L.ah_last_error().decode()
    status, text = call_batch(L, [bad, None, EMPTY])  # the NULL blob before the malformed one in front of it
    assert status == 5 and "blobs[1] is NULL" in text, text


@pytest.mark.parametrize("name", sorted(malformations()))
def test_every_malformed_header_is_refused_with_its_position(name):
    from arroy_amd import _lib
    L = _lib.lib()
    blob, container, word = malformations()[name]
    with pytest.raises(ValueError):
        roaring.deserialize(blob)
    good = [roaring.serialize(corpus()["nine_keys"], runs=True), roaring.serialize(corpus()["bitmap_4097"])]
    for pos in (0, 2):
        batch = list(good)
        batch.insert(pos, blob)
        status, text = call_batch(L, batch)
        assert status == 5 and f"blobs[{pos}]:" in text and word in text and "index is NULL" not in text, (name, pos, text)
        assert re.findall(r"container (\d+):", text) == ([str(container)] if container is not None else []), text
    a = np.frombuffer(blob, dtype=np.uint8)
    h = C.c_void_p(0xDEAD)
    assert L.ah_filter_create_roaring(None, a.ctypes.data, a.size, C.byref(h)) == 5 and h.value is None
    assert "blobs[0]:" in L.ah_last_error().decode() and word in L.ah_last_error().decode()
