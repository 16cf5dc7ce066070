"""plan_chunk under AH_SEARCH_TILES_MANHATTAN (arroy_amd/csrc/search_plan.h): a stand-alone program
(tests/search_manhattan_plan_check.cpp, its own main, no device call) built with AddressSanitizer and UBSan."""
import os
import subprocess

from conftest import ROOT
from test_index_workspace_cpu import compilers

SRC = os.path.join(ROOT, "tests", "search_manhattan_plan_check.cpp")


def test_manhattan_plans_as_euclidean_under_the_knob(tmp_path):
    exe = str(tmp_path / "search_manhattan_plan_check")
    tried = []
    for cxx in compilers():
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all", "-pthread", SRC, "-o", exe], capture_output=True, text=True)
        if build.returncode == 0:
            break
        tried.append(f"{cxx}: {build.stderr[-2000:]}")
    else:
        raise AssertionError("no host compiler built the sanitized program:\n" + "\n".join(tried))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "planned where they should be" in run.stdout and run.stderr == "", run.stdout + run.stderr
