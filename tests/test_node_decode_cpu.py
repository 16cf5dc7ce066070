"""The node decoder (arroy_amd/csrc/node_decode.h) without a GPU: tests/node_decode_check.cpp — a stand-alone program, its own
main, no device call — is built with AddressSanitizer and UBSan and run directly.  It feeds the decoder a corpus of values
whole, as every prefix and under single-byte mutations, each in an allocation of exactly its length at offsets 0 to 3, and
prints what measure_value and decode_descendants make of every whole value; that is compared here with the plain restatement
arroy_amd/node_codec.py and with the id sets the values were made from.  Also what of ah_index_create_from_encoded needs no
device: the symbol, the prototype and the argument checks."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import node_codec_cases as cases
from conftest import ROOT
from test_index_workspace_cpu import compilers

from arroy_amd import distances as D
from arroy_amd import node_codec

SRC = os.path.join(ROOT, "tests", "node_decode_check.cpp")
FIELDS = ("reason", "kind", "has_normal", "left", "right", "ids", "containers", "arrays", "bitmaps", "runs", "content")
CONTENT_REASONS = range(11, 16)  # R_ARRAY_ORDER .. R_RUN_CARDINALITY of node_decode.h


@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("node_decode")
    exe = str(tmp / "node_decode_check")
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
        assert "# every accepted value decodes inside its bytes and its count" in out.stdout
        rows = []
        for text in out.stdout.splitlines():
            if text.startswith("#"):
                continue
            words = [int(w) for w in text.split()]
            row = dict(zip(FIELDS, words))
            row["list"] = np.array(words[len(FIELDS):], dtype=np.uint32)
            rows.append(row)
        return rows
    return run


def value_line(value: bytes, hs: int = 4, vs: int = 120) -> str:
    return "V %d %d %s" % (hs, vs, bytes(value).hex() or "-")


def ids_line(ids) -> str:
    return "I %d %s" % (len(ids), " ".join(str(int(x)) for x in ids))


def check_against_python(row, distance, dims, value):
    """One printed row against node_codec.decode_value of the same bytes (12346 values and split values)."""
    try:
        want = node_codec.decode_value(distance, dims, value)
    except (ValueError, struct.error, IndexError):
        want = None
    if want is None:
        assert row["reason"] != 0 or row["content"] != 0, value[:16].hex()
        return
    assert row["reason"] == 0 and row["content"] == 0, (row["reason"], row["content"], value[:16].hex())
    if want[0] == "S":
        assert (row["kind"], row["left"], row["right"], row["has_normal"]) == (2, want[1], want[2], int(want[3] is not None))
    else:
        assert row["kind"] == 1 and row["ids"] == want[1].size and np.array_equal(row["list"], want[1])
        assert row["containers"] == np.unique(want[1] >> 16).size == row["arrays"] + row["bitmaps"] and row["runs"] == 0


def test_fixture_values_decode_to_what_roaring_wrote(host_decoder):
    values = cases.fixture_descendants()
    assert len(values) == 59
    rows = host_decoder([value_line(v, 4, 120) for v in values])
    assert len(rows) == 59
    for row, v in zip(rows, values):
        check_against_python(row, D.Euclidean, 30, v)
    assert sorted(r["ids"] for r in rows)[0] == 0  # the empty list among them


def test_edge_sets_in_both_cookie_forms(host_decoder):
    sets = dict(cases.edge_lists(), containers_300=cases.containers_300())
    # run containers where they pay: one long run, many short runs, and fewer than / at least 4 containers of them
    sets["run_full"] = np.arange(7 << 16, 8 << 16, dtype=np.uint32)
    sets["runs_2048"] = (np.arange(2048, dtype=np.uint32) * 2 + (1 << 16)).astype(np.uint32)
    sets["runs_3_containers"] = np.concatenate([np.arange(10, 500) + (k << 16) for k in (1, 4, 9)]).astype(np.uint32)
    sets["runs_5_containers"] = np.concatenate([np.arange(k, 300 + 7 * k) + (k << 16) for k in range(5)]).astype(np.uint32)
    names = list(sets)
    rows = host_decoder([ids_line(sets[k]) for k in names])
    assert len(rows) == 2 * len(names)
    saw_runs_below_4 = saw_runs_from_4 = False
    for i, name in enumerate(names):
        ids = sets[name]
        plain, runs = rows[2 * i], rows[2 * i + 1]
        check_against_python(plain, D.Euclidean, 30, node_codec.encode_descendants(ids))
        keys = np.unique(ids >> 16).size
        for row in (plain, runs):
            assert (row["reason"], row["content"], row["kind"], row["ids"]) == (0, 0, 1, ids.size), name
            assert np.array_equal(row["list"], ids), name
            assert row["containers"] == keys == row["arrays"] + row["bitmaps"] + row["runs"], name
        if runs["runs"]:
            saw_runs_below_4 |= keys < 4
            saw_runs_from_4 |= keys >= 4
    assert saw_runs_below_4 and saw_runs_from_4  # the 12347 form without and with its offset header
    by = {name: rows[2 * i + 1] for i, name in enumerate(names)}
    assert by["run_full"]["runs"] == 1 and by["runs_2048"]["runs"] == 0  # 2048 runs of one: the array is smaller
    assert by["full_container"]["runs"] == 1 and by["bitmap_4097"]["bitmaps"] == 1 and by["array_4096"]["arrays"] == 1


@pytest.mark.parametrize("dims", [30, 64])
def test_split_values_and_refusals(host_decoder, dims):
    rng = np.random.default_rng(dims)
    lines, meta = [], []
    for dist in (D.Euclidean, D.DotProduct, D.BinaryQuantizedCosine):  # header sizes 4 and 8, f32 and 1-bit vectors
        hs, vs = dist.header_size(), dist.vector_size(dims)
        assert hs == (8 if dist is D.DotProduct else 4)
        normal = rng.integers(0, 256, size=hs + vs, dtype=np.uint8).tobytes()
        good = [node_codec.encode_split(1, 2, normal), node_codec.encode_split(0x01020304, 0xFFFFFFFE, None)]
        bad = [good[0][:-1], good[0] + b"\0", good[1] + b"\0", b"\0" + good[0][1:], b"\7" + good[1][1:], b""]
        for v in good + bad:
            lines.append(value_line(v, hs, vs))
            meta.append((dist, v, v in good))
    rows = host_decoder(lines)
    for row, (dist, v, ok) in zip(rows, meta):
        assert (row["reason"] == 0) == ok, (dist.__name__, len(v))
        if v:
            check_against_python(row, dist, dims, v)
    # Descendants values node_codec.decode_value refuses: the cookie, a trailing byte, a short value, a wrong offset entry
    good = node_codec.encode_descendants(np.array([1, 5, 70000, 70001], np.uint32))
    wrong_cookie = good[:1] + struct.pack("<I", 12345) + good[5:]
    wrong_offset = good[:17] + struct.pack("<I", 25) + good[21:]
    keys_descend = good[:9] + good[13:17] + good[9:13] + good[17:]
    bad = [wrong_cookie, good + b"\0", good[:-1], wrong_offset, keys_descend]
    rows = host_decoder([value_line(v) for v in [good] + bad])
    assert rows[0]["reason"] == 0 and rows[0]["list"].tolist() == [1, 5, 70000, 70001]
    assert [r["reason"] for r in rows[1:]] == [5, 9, 7, 8, 6]  # R_COOKIE, R_TRAILING, R_PAST_END, R_OFFSET, R_KEY_ORDER
    # content: an array that does not ascend (the headers are fine)
    unsorted = good[:25] + struct.pack("<HH", 5, 5) + good[29:]
    rows = host_decoder([value_line(unsorted)])
    assert rows[0]["reason"] == 0 and rows[0]["content"] in CONTENT_REASONS


def test_the_library_exports_the_decoder_and_judges_its_arguments():
    from arroy_amd import _lib
    L = _lib.lib()
    assert "ah_index_create_from_encoded" in _lib.SIGNATURES and L.ah_index_create_from_encoded is not None
    with open(os.path.join(ROOT, "include", "arroy_hip.h")) as f:
        header = f.read()
    assert "ah_index_create_from_encoded(" in header and "ah_index_decode_stats" in header
    assert _lib.tuning_get("AH_DECODE_CHUNK_BYTES") == (64 << 20, 64 << 20)
    # out NULL, dataset NULL: refused before any device is touched, *out left NULL
    INVALID = 5
    h = C.c_void_p(77)
    assert L.ah_index_create_from_encoded(None, None, None, None, 0, None, 0, None, None) == INVALID and b"out is NULL" in L.ah_last_error()
    assert L.ah_index_create_from_encoded(None, None, None, None, 0, None, 0, C.byref(h), None) == INVALID
    assert b"dataset is NULL" in L.ah_last_error() and h.value is None
