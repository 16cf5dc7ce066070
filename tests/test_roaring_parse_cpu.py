"""The host parser of serialized RoaringBitmaps (arroy_amd/csrc/roaring_parse.h), checked on the host: a stand-alone program
(tests/roaring_parse_check.cpp, its own main, no device call) built with AddressSanitizer and UBSan feeds it a valid corpus in
both cookie forms, every prefix of it, a few thousand single-byte mutations and blobs at odd addresses, each in an allocation
of exactly its length, and expects a descriptor list whose ranges lie inside the blob or a refusal."""
import os
import subprocess

from conftest import ROOT
from test_index_workspace_cpu import compilers

SRC = os.path.join(ROOT, "tests", "roaring_parse_check.cpp")


def test_the_parser_stays_inside_every_blob(tmp_path):
    exe = str(tmp_path / "roaring_parse_check")
    tried = []
    for cxx in compilers():
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                SRC, "-o", exe], capture_output=True, text=True)
        if build.returncode == 0:
            break
        tried.append(f"{cxx}: {build.stderr[-2000:]}")
    else:
        raise AssertionError("no host compiler built the sanitized program:\n" + "\n".join(tried))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every accepted blob has its containers inside it" in run.stdout and run.stderr == "", run.stdout + run.stderr
