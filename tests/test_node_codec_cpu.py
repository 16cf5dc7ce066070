"""The node codec (arroy_amd/csrc/node_codec.h, arroy_amd/node_codec.py) without a GPU: the bytes `NodeCodec` stores for a
tree node (src/node.rs:229-241).  tests/node_codec_check.cpp — a stand-alone program, its own main, no device call — is built
with AddressSanitizer and UBSan and run directly; its values are compared byte for byte with the Python restatement and with
what roaring-rs itself wrote into tests/golden/large_v0_6.mdb."""
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

SRC = os.path.join(ROOT, "tests", "node_codec_check.cpp")
METRICS = [D.Euclidean, D.Manhattan, D.Cosine, D.DotProduct, D.BinaryQuantizedEuclidean, D.BinaryQuantizedManhattan,
           D.BinaryQuantizedCosine]


@pytest.fixture(scope="module")
def host_encoder(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("node_codec") / "node_codec_check")
    tried = []
    for cxx in compilers():
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
        if build.returncode == 0:
            break
        tried.append(f"{cxx}: {build.stderr[-2000:]}")
    else:
        raise AssertionError("no host compiler built the sanitized program:\n" + "\n".join(tried))

    def run(lines, tmp_path):
        path = os.path.join(str(tmp_path), "cases.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        values = [bytes.fromhex(h) for h in out.stdout.split()]
        assert len(values) == len(lines), (len(values), len(lines), out.stderr)
        return values
    return run


def desc_line(ids):
    return "D %d %s" % (len(ids), " ".join(str(int(x)) for x in ids))


def test_fixture_values_reencode_to_the_same_bytes(host_encoder, tmp_path):
    values = cases.fixture_descendants()
    assert len(values) == 59
    lists = [node_codec.decode_value(D.Euclidean, 30, v)[1] for v in values]
    sizes = sorted(len(l) for l in lists)
    assert sizes[0] == 0 and sizes[-1] == 30, sizes  # an empty list is among them
    assert [node_codec.encode_descendants(l) for l in lists] == values
    assert host_encoder([desc_line(l) for l in lists], tmp_path) == values


def test_host_encoder_agrees_with_the_python_one_at_every_container_rule(host_encoder, tmp_path):
    lists = dict(cases.edge_lists(), containers_300=cases.containers_300())
    names = list(lists)
    got = host_encoder([desc_line(lists[k]) for k in names], tmp_path)
    for name, value in zip(names, got):
        ids = lists[name]
        assert value == node_codec.encode_descendants(ids), name
        kind, back = node_codec.decode_value(D.Euclidean, 30, value)
        assert kind == "D" and np.array_equal(back, ids), name
        # every size formula against the written length
        keys, cards = np.unique(ids >> 16, return_counts=True)
        body = sum(2 * int(c) if c <= 4096 else 8192 for c in cards)
        assert len(value) == 1 + 8 + 8 * len(keys) + body <= node_codec.descendants_value_bound(len(ids)), name
        cookie, nc = struct.unpack("<II", value[1:9])
        assert (cookie, nc) == (12346, len(keys)), name
    by = dict(zip(names, got))
    assert len(by["empty"]) == 9
    assert len(by["array_4096"]) == 1 + 8 + 8 + 2 * 4096     # 4096 ids in one container: an array
    assert len(by["bitmap_4097"]) == 1 + 8 + 8 + 8192         # 4097: a bitmap
    assert len(by["neighbours_65535_65536"]) == 1 + 8 + 16 + 4  # two containers of one id
    assert struct.unpack("<I", by["containers_300"][5:9])[0] == 300
    assert len(by["bitmap_array_one"]) == 1 + 8 + 24 + 8192 + 8192 + 2
    with pytest.raises(ValueError):
        node_codec.encode_descendants([3, 3])
    with pytest.raises(ValueError):
        node_codec.encode_descendants([4, 3])


@pytest.mark.parametrize("dims", [30, 64])
def test_split_values_of_every_metric(host_encoder, tmp_path, dims):
    rng = np.random.default_rng(dims)
    lines, want, meta = [], [], []
    for dist in METRICS:
        hs, vs = dist.header_size(), dist.vector_size(dims)
        normal = rng.integers(0, 256, size=hs + vs, dtype=np.uint8).tobytes()
        for left, right, nb in ((1, 2, normal), (0x01020304, 0x01020305, normal), (0x01020304 + 7, 0xFFFFFFFE, None)):
            lines.append("S %d %d %d %d %s" % (left, right, hs, vs, nb.hex() if nb is not None else "-"))
            want.append(node_codec.encode_split(left, right, nb))
            meta.append((dist, left, right, nb))
    got = host_encoder(lines, tmp_path)
    assert got == want
    for value, (dist, left, right, nb) in zip(got, meta):
        assert len(value) == node_codec.split_value_len(nb is not None, dist.header_size(), dist.vector_size(dims))
        assert len(value) == (9 if nb is None else 9 + dist.header_size() + dist.vector_size(dims))
        assert value[0] == 2 and value[1:5] == left.to_bytes(4, "big") and value[5:9] == right.to_bytes(4, "big")
        assert node_codec.decode_value(dist, dims, value) == ("S", left, right, nb)
    assert want[1][1:9] == bytes([1, 2, 3, 4, 1, 2, 3, 5])  # base 0x01020304, big-endian


def build_stream_encoded_example(tmp_path):
    """examples/stream_encoded.c as strict C99 (it looks the encoded entry point up at run time: -ldl)."""
    exe = str(tmp_path / "stream_encoded")
    lib_dir = os.path.join(ROOT, "arroy_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "stream_encoded.c"), "-o", exe, "-L", lib_dir, "-larroy_hip", "-ldl",
                           f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_stream_encoded_example_compiles_and_explains_itself(tmp_path):
    exe = build_stream_encoded_example(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "host|encoded|empty" in out.stderr


def test_the_library_exports_the_encoded_stream():
    from arroy_amd import _lib
    lib = _lib.lib()
    for name in ("ah_build_forest_stream_encoded", "ah_encode_descendants"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    with open(os.path.join(ROOT, "include", "arroy_hip.h")) as f:
        header = f.read()
    assert "ah_build_forest_stream_encoded(" in header and "ah_encode_descendants(" in header and "ah_encode_options" in header
