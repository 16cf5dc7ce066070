"""The v0.4 - v0.6 node layouts without a GPU.  The host rules (arroy_amd/csrc/node_legacy.h) as a stand-alone program:
tests/node_legacy_check.cpp — its own main, no device call — is built with AddressSanitizer and UBSan, exactly as
tests/test_node_decode_cpu.py builds its checker, and run directly; what it prints is compared with the plain restatement
arroy_amd/node_codec.py.  Then node_codec.upgrade_values on the two v0.6 fixtures against the dumps the reference's own
upgrade tests assert (tests/golden/upgrade_expected.json), and what of ah_index_create_from_legacy needs no device."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import node_legacy_cases as legacy_cases
from conftest import ROOT
from test_index_workspace_cpu import compilers

from arroy_amd import distances as D
from arroy_amd import node_codec

SRC = os.path.join(ROOT, "tests", "node_legacy_check.cpp")
FIELDS = ("reason", "kind", "has_normal", "left", "right", "left_is_item", "right_is_item", "ids")
R_SPLIT_LEN_LEGACY, R_CHILD_MODE = 18, 19  # behind R_ROOT_ABSENT = 17 of node_decode.h
R_EMPTY, R_TAG = 1, 2


@pytest.fixture(scope="module")
def host_rules(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("node_legacy")
    exe = str(tmp / "node_legacy_check")
    tried = []
    for cxx in compilers():
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
        if build.returncode == 0:
            break
        tried.append(f"{cxx}: {build.stderr[-2000:]}")
    else:
        raise AssertionError("no host compiler built the sanitized program:\n" + "\n".join(tried))
    calls = []

    def run(lines):
        path = str(tmp / f"cases{len(calls)}.txt")
        calls.append(path)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
        assert out.stderr == "", out.stderr[-4000:]
        assert "# every accepted legacy value keeps the rules of its layout" in out.stdout
        rows = []
        for text in out.stdout.splitlines():
            if text.startswith("#"):
                continue
            words = text.split(" ", len(FIELDS))
            if len(words) == 1:
                rows.append(int(words[0]))  # a Z line
                continue
            row = dict(zip(FIELDS, (int(w) for w in words[:len(FIELDS)])))
            row["text"] = words[len(FIELDS)] if len(words) > len(FIELDS) else ""
            rows.append(row)
        return rows
    return run


def value_line(layout, dist, dims, value: bytes) -> str:
    return "L %d %d %d %s" % (node_codec.layout_of(layout), 0 if dist.binary_quantized else 1, dist.vector_size(dims), bytes(value).hex() or "-")


def check_against_python(row, layout, dist, dims, value):
    try:
        want = node_codec.decode_legacy_value(layout, dist, dims, value)
    except (ValueError, struct.error, IndexError):
        want = None
    if want is None:
        assert row["reason"] != 0, value[:16].hex()
        return
    assert row["reason"] == 0, (row, value[:16].hex())
    if want[0] == "S":
        assert (row["kind"], row["left"], row["right"]) == (2, want[1][1], want[2][1])
        assert (row["left_is_item"], row["right_is_item"]) == (int(want[1][0] == "item"), int(want[2][0] == "item"))
        assert row["has_normal"] == int(want[3] is not None)
    else:
        assert row["kind"] == 1 and row["ids"] == want[1].size


F32 = struct.Struct("<f")


def f32_vectors(dims):
    """name -> (vector bytes, is_zero): +0.0, -0.0, a mix of the two, one denormal, one NaN, an ordinary normal."""
    plus, minus = F32.pack(0.0), F32.pack(-0.0)
    mix = b"".join(minus if i % 3 == 1 else plus for i in range(dims))
    denormal = plus * (dims - 1) + struct.pack("<I", 1)              # the smallest positive denormal, in the last element
    minus_denormal = struct.pack("<I", 0x80000001) + minus * (dims - 1)
    nan = minus * (dims // 2) + struct.pack("<I", 0x7FC00000) + plus * (dims - dims // 2 - 1)
    ordinary = np.random.default_rng(dims).standard_normal(dims).astype("<f4").tobytes()
    return {"plus": (plus * dims, True), "minus": (minus * dims, True), "mix": (mix, True), "denormal": (denormal, False),
            "minus_denormal": (minus_denormal, False), "nan": (nan, False), "ordinary": (ordinary, False)}


@pytest.mark.parametrize("dims", [1, 7, 30])
def test_the_zero_test_of_f32_vectors(host_rules, dims):
    vectors = f32_vectors(dims)
    rows = host_rules(["Z 1 %s" % v.hex() for v, _ in vectors.values()])
    for (name, (v, zero)), got in zip(vectors.items(), rows):
        assert got == int(zero), name
        assert node_codec.vector_is_zero(D.Euclidean, v) == zero, name
        # the same bytes as a binary-quantized vector: zero only when every byte is (-0.0 has a byte 0x80)
        assert node_codec.vector_is_zero(D.BinaryQuantizedEuclidean, v) == (not any(v)), name
    rows = host_rules(["Z 0 %s" % v.hex() for v, _ in vectors.values()])
    assert rows == [int(not any(v)) for v, _ in vectors.values()] and rows[0] == 1 and rows[1] == 0


@pytest.mark.parametrize("layout", ["v0.5", "v0.4"])
def test_split_values_of_both_mode_numberings(host_rules, layout):
    """Every pair of child modes, every kind of vector, f32 and binary-quantized rows (one and two 64-bit words), against the
    Python restatement; the mode bytes of the OTHER numbering and every other byte value are refused."""
    modes = node_codec.legacy_modes(layout)
    assert modes == ({"tree": 2, "item": 3} if layout == "v0.5" else {"tree": 1, "item": 0})
    lines, meta = [], []
    for dist, dims in ((D.Euclidean, 7), (D.Cosine, 30), (D.DotProduct, 2), (D.BinaryQuantizedCosine, 64), (D.BinaryQuantizedEuclidean, 100)):
        vs = dist.vector_size(dims)
        if dist.binary_quantized:
            vectors = {"zero": (b"\0" * vs, True), "one_bit": (b"\0" * (vs - 1) + b"\x80", False), "ones": (b"\xff" * vs, False)}
        else:
            vectors = f32_vectors(dims)
        for lm in ("tree", "item"):
            for rm in ("tree", "item"):
                for name, (vec, zero) in vectors.items():
                    v = node_codec.encode_split_legacy(layout, (lm, 0x01020304), (rm, 0xFFFFFFFE), vec)
                    assert len(v) == 11 + vs
                    lines.append(value_line(layout, dist, dims, v))
                    meta.append((dist, dims, v, zero))
    rows = host_rules(lines)
    assert len(rows) == len(meta)
    for row, (dist, dims, v, zero) in zip(rows, meta):
        assert row["reason"] == 0 and row["has_normal"] == int(not zero)
        check_against_python(row, layout, dist, dims, v)
    # refusals, by reason
    dist, dims = D.Euclidean, 7
    vec = f32_vectors(dims)["ordinary"][0]
    good = node_codec.encode_split_legacy(layout, ("tree", 1), ("item", 2), vec)
    other = node_codec.legacy_modes("v0.4" if layout == "v0.5" else "v0.5")
    v07 = node_codec.encode_split(1, 2, b"\0" * 4 + vec)
    cases = [
        (good[:-1], R_SPLIT_LEN_LEGACY), (good + b"\0", R_SPLIT_LEN_LEGACY), (good[:9], R_SPLIT_LEN_LEGACY), (good[:11], R_SPLIT_LEN_LEGACY),
        (v07, R_SPLIT_LEN_LEGACY),  # 9 + header + vector: the v0.7 layout under a legacy one
        (node_codec.encode_split_legacy(layout, (other["tree"], 1), ("tree", 2), vec), R_CHILD_MODE),
        (node_codec.encode_split_legacy(layout, ("tree", 1), (other["item"], 2), vec), R_CHILD_MODE),
        (node_codec.encode_split_legacy(layout, (4, 1), ("tree", 2), vec), R_CHILD_MODE),
        (node_codec.encode_split_legacy(layout, ("item", 1), (255, 2), vec), R_CHILD_MODE),
        (b"", R_EMPTY), (b"\0" + good[1:], R_TAG), (b"\7" + good[1:], R_TAG),
    ]
    rows = host_rules([value_line(layout, dist, dims, v) for v, _ in cases])
    assert [r["reason"] for r in rows] == [want for _, want in cases]
    assert "11 + vector" in rows[0]["text"] and "mode byte" in rows[5]["text"] and "unknown node tag" in rows[-1]["text"]
    for row, (v, _) in zip(rows, cases):
        if v:
            check_against_python(row, layout, dist, dims, v)
    # Descendants values are those of v0.7
    desc = node_codec.encode_descendants(np.array([1, 5, 70000], np.uint32))
    rows = host_rules([value_line(layout, dist, dims, desc), value_line(layout, dist, dims, desc[:-1])])
    assert (rows[0]["reason"], rows[0]["kind"], rows[0]["ids"]) == (0, 1, 3) and rows[1]["reason"] != 0


def test_the_fixture_values_through_the_host_rules(host_rules):
    for name in ("smol", "large"):
        dims, _ids, _vecs, node_ids, values, _roots = legacy_cases.fixture(name)
        rows = host_rules([value_line("v0.6", D.Euclidean, dims, v) for v in values])
        for row, v in zip(rows, values):
            check_against_python(row, "v0.6", D.Euclidean, dims, v)
        splits = [r for r, v in zip(rows, values) if v[0] == 2]
        if name == "smol":
            assert len(splits) == 3 and sum(1 - r["has_normal"] for r in splits) == 2
            assert sum(r["left_is_item"] + r["right_is_item"] for r in splits) == 2
        else:
            assert len(splits) == 49 and all(len(v) == 131 for v in values if v[0] == 2)
            assert all(r["has_normal"] and not r["left_is_item"] and not r["right_is_item"] for r in splits)


# ---- node_codec.upgrade_values on the fixtures --------------------------------------------------------------------------------
def test_upgrade_values_of_smol_is_the_reference_dump():
    dims, _ids, _vecs, node_ids, values, roots = legacy_cases.fixture("smol")
    assert node_ids == [0, 1, 2, 3, 4] and roots == [0]
    new_ids, new_values, put = node_codec.upgrade_values("v0.6", node_ids, values, D.Euclidean, dims)
    assert new_ids == [0, 1, 2, 3, 4, 5, 6] and put == [5, 0, 6, 3, 4]
    dec = {n: node_codec.decode_value(D.Euclidean, dims, v) for n, v in zip(new_ids, new_values)}
    one_zero = struct.pack("<fff", 0.0, 1.0, 0.0)  # bias 0, then the normal [1, 0]
    assert dec[0] == ("S", 5, 4, one_zero)
    assert dec[3] == ("S", 2, 6, None) and dec[4] == ("S", 1, 3, None)
    assert dec[5][0] == "D" and dec[5][1].tolist() == [0] and dec[6][0] == "D" and dec[6][1].tolist() == [2]
    assert new_values[1] == values[1] and new_values[2] == values[2]  # Descendants values: not touched
    assert legacy_cases.records(D.Euclidean, dims, new_ids, new_values) == legacy_cases.expected()["smol"]["trees"]


def test_upgrade_values_of_large_is_the_reference_dump():
    dims, _ids, _vecs, node_ids, values, roots = legacy_cases.fixture("large")
    new_ids, new_values, put = node_codec.upgrade_values("v0.6", node_ids, values, D.Euclidean, dims)
    assert len(new_ids) == 108 and new_ids == node_ids, "no new node"
    splits = [n for n, v in zip(node_ids, values) if v[0] == 2]
    assert put == splits and len(splits) == 49
    assert all(len(v) == 9 + 4 + 120 for v in new_values if v[0] == 2), "no zero normal"
    assert all(v[9:13] == b"\0\0\0\0" for v in new_values if v[0] == 2), "a Euclidean bias is 0"
    assert legacy_cases.records(D.Euclidean, dims, new_ids, new_values) == legacy_cases.expected()["large"]["trees"]
    assert roots == [8, 17, 24, 35, 44, 55, 64, 75, 86, 97]


def test_upgrade_values_makes_the_cosine_norm_and_keeps_v0_7_values():
    rng = np.random.default_rng(3)
    vec = rng.standard_normal(30).astype("<f4")
    legacy = [node_codec.encode_split_legacy("v0.4", ("item", 9), ("item", 4), vec.tobytes()), node_codec.encode_descendants([1, 2])]
    ids, values, put = node_codec.upgrade_values("v0.4", [10, 20], legacy, D.Cosine, 30)
    assert ids == [10, 20, 21, 22] and put == [21, 22, 10]
    kind, left, right, normal = node_codec.decode_value(D.Cosine, 30, values[0])
    assert (kind, left, right) == ("S", 21, 22) and normal[4:] == vec.tobytes()
    norm = np.frombuffer(normal[:4], "<f4")[0]
    assert abs(float(norm) - float(np.sqrt(np.sum(vec.astype(np.float64) ** 2)))) < 1e-5 * float(norm)
    assert [node_codec.decode_value(D.Cosine, 30, v)[1].tolist() for v in values[2:]] == [[9], [4]]
    bq = node_codec.encode_split_legacy("v0.5", ("tree", 20), ("tree", 20), b"\x01" + b"\0" * 15)
    _ids, values, _put = node_codec.upgrade_values("v0.5", [10, 20], [bq, legacy[1]], D.BinaryQuantizedCosine, 100)
    assert np.frombuffer(values[0][9:13], "<f4")[0] == np.float32(np.sqrt(np.float32(128.0)))  # bq_cosine.rs:45-47: the norm of +-1 in every stored bit
    same = node_codec.upgrade_values("v0.7", [10, 20], [values[0], legacy[1]], D.BinaryQuantizedCosine, 100)
    assert same == ([10, 20], [values[0], legacy[1]], [])
    with pytest.raises(ValueError):
        node_codec.upgrade_values("v0.3", [1], [legacy[1]], D.Cosine, 30)
    with pytest.raises(ValueError):
        node_codec.decode_legacy_value("v0.5", D.Cosine, 30, legacy[0])  # v0.4 mode bytes under v0.5


# ---- the entry point without a device --------------------------------------------------------------------------------------------
def test_the_library_exports_the_legacy_open_and_judges_its_arguments():
    from arroy_amd import _lib
    L = _lib.lib()
    assert "ah_index_create_from_legacy" in _lib.SIGNATURES and L.ah_index_create_from_legacy is not None
    assert len(_lib.SIGNATURES["ah_index_create_from_legacy"][1]) == 11
    with open(os.path.join(ROOT, "include", "arroy_hip.h")) as f:
        header = f.read()
    assert "ah_index_create_from_legacy(" in header and "ah_index_legacy_stats" in header
    for name, value in (("AH_NODE_LAYOUT_V0_7", 0), ("AH_NODE_LAYOUT_V0_5", 1), ("AH_NODE_LAYOUT_V0_4", 2)):
        assert f"{name} = {value}" in header
    assert (_lib.NODE_LAYOUT_V0_7, _lib.NODE_LAYOUT_V0_5, _lib.NODE_LAYOUT_V0_4) == (0, 1, 2)
    assert _lib.NODE_LAYOUTS == node_codec.LAYOUTS and _lib.NODE_LAYOUTS["v0.6"] == _lib.NODE_LAYOUTS["v0.5"] == 1
    assert C.sizeof(_lib.AhIndexLegacyStats) == 5 * 8 and C.sizeof(_lib.AhIndexDecodeStats) == 12 * 8 + 2 * 8
    INVALID = 5
    h = C.c_void_p(77)
    legacy = _lib.AhIndexLegacyStats(1, 2, 3, 4, 5)
    assert L.ah_index_create_from_legacy(None, 1, None, None, None, 0, None, 0, None, None, None) == INVALID and b"out is NULL" in L.ah_last_error()
    for layout in (-1, 3, 7):
        h.value = 77
        assert L.ah_index_create_from_legacy(None, layout, None, None, None, 0, None, 0, C.byref(h), None, C.byref(legacy)) == INVALID
        assert b"unknown node layout" in L.ah_last_error() and h.value is None and legacy.new_nodes == 0
    for layout in (0, 1, 2):
        h.value = 77
        assert L.ah_index_create_from_legacy(None, layout, None, None, None, 0, None, 0, C.byref(h), None, None) == INVALID
        assert b"dataset is NULL" in L.ah_last_error() and h.value is None
