"""The host side of ah_index_drop_trees (`delete_extra_trees`, src/writer.rs:631-655, on a resident index) without a GPU: the
root arithmetic both paths of ArroyBuilder._incremental share (index.roots_after_drop) against a literal restatement of the
reference's loop, and the call's workspace layout (drop_workspace, arroy_amd/csrc/index_workspace.h) carved and filled by a
stand-alone program (tests/index_drop_workspace_check.cpp, its own main, no device call) built with AddressSanitizer and
UBSan."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

from arroy_amd.index import roots_after_drop

SRC = os.path.join(ROOT, "tests", "index_drop_workspace_check.cpp")


def reference_loop(roots, n_trees_to_remove):
    """The loop of `delete_extra_trees`: as many times as there are extraneous trees, stop when the roots are empty, else
    `roots.swap_remove(0)` and delete that tree.  Vec::swap_remove spelt out: the element is taken out and the LAST element
    is put in its place."""
    roots, deleted = list(roots), []
    for _ in range(n_trees_to_remove):
        if not roots:
            break
        last = roots.pop()          # swap_remove(0): the last element ...
        if roots:
            removed, roots[0] = roots[0], last   # ... takes the place of the first, which is returned
        else:
            removed = last
        deleted.append(removed)
    return roots, deleted


@pytest.mark.parametrize("n", range(10))
def test_roots_after_drop_is_the_reference_loop(n):
    roots = [10 + 7 * t for t in range(n)]
    for n_drop in range(n + 3):
        before = list(roots)
        kept, dropped = roots_after_drop(roots, n_drop)
        assert roots == before  # (a pure function)
        assert (kept, dropped) == reference_loop(roots, n_drop), (n, n_drop)
        assert len(dropped) == min(n, n_drop) and sorted(kept + dropped) == roots


def test_roots_after_drop_pinned():
    r = ["r0", "r1", "r2", "r3", "r4", "r5"]
    assert roots_after_drop(r, 4) == (["r2", "r1"], ["r0", "r5", "r4", "r3"])
    assert roots_after_drop(r, 0) == (r, [])
    assert roots_after_drop(r, 6) == ([], ["r0", "r5", "r4", "r3", "r2", "r1"])
    assert roots_after_drop(r, 8) == roots_after_drop(r, 6)
    assert roots_after_drop([], 3) == ([], [])


def compilers():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx) if cxx else None
        if path:
            yield path


def test_the_drop_layout_lies_inside_its_block(tmp_path):
    exe = str(tmp_path / "index_drop_workspace_check")
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
    assert "every array inside its block" in run.stdout and run.stderr == "", run.stdout + run.stderr
