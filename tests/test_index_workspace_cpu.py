"""The workspace layouts of the index maintenance calls (arroy_amd/csrc/index_workspace.h), checked on the host: a stand-alone
program (tests/index_workspace_check.cpp, its own main, no device call) built with AddressSanitizer and UBSan carves every
layout for sizes from 0 up, fills every array and compares the block and its zeroed part with the formulas the calls used
before the layouts were written down once."""
import os
import shutil
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "index_workspace_check.cpp")


def compilers():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx) if cxx else None
        if path:
            yield path


def test_every_layout_lies_inside_its_block(tmp_path):
    exe = str(tmp_path / "index_workspace_check")
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
    assert "every layout inside its block" in run.stdout and run.stderr == "", run.stdout + run.stderr
