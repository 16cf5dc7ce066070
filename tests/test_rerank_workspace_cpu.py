"""The device and pinned layouts of a sub-batch of ah_rerank_batch (arroy_amd/csrc/rerank_workspace.h), checked on the host: a
stand-alone program (tests/rerank_workspace_check.cpp, its own main, no device call) built with AddressSanitizer and UBSan
counts every layout, carves it into a heap block of exactly that size for sizes from 0 to a sub-batch's limits, touches every
array and compares the bytes with the sums the call kept by hand before the layouts were written down once."""
import os
import subprocess

from conftest import ROOT
from test_index_workspace_cpu import compilers

SRC = os.path.join(ROOT, "tests", "rerank_workspace_check.cpp")


def test_every_rerank_layout_lies_inside_its_block(tmp_path):
    exe = str(tmp_path / "rerank_workspace_check")
    tried = []
    for cxx in compilers():
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                                SRC, "-o", exe], capture_output=True, text=True)
        if build.returncode == 0:
            break
        tried.append(f"{cxx}: {build.stderr[-2000:]}")
    else:
        raise AssertionError("no host compiler built the sanitized program:\n" + "\n".join(tried))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every layout inside its block" in run.stdout and run.stderr == "", run.stdout + run.stderr
