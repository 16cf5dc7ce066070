"""ChunkPlan::flag_slices (arroy_amd/csrc/search_plan.h, AH_SEARCH_FLAG_SLICED) at every one of its host-checked conditions: a
stand-alone program (tests/search_flag_sliced_plan_check.cpp, its own main, no device call) built with AddressSanitizer and UBSan."""
import os
import subprocess

from conftest import ROOT
from test_index_workspace_cpu import compilers


def test_sliced_flags_are_planned_where_they_should_be(tmp_path):
    src, exe, tried = os.path.join(ROOT, "tests", "search_flag_sliced_plan_check.cpp"), str(tmp_path / "search_flag_sliced_plan_check"), []
    for cxx in compilers():
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all", "-pthread", src, "-o", exe], capture_output=True, text=True)
        if build.returncode == 0:
            break
        tried.append(f"{cxx}: {build.stderr[-2000:]}")
    else:
        raise AssertionError("no host compiler built the sanitized program:\n" + "\n".join(tried))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "planned where they should be" in run.stdout and run.stderr == "", run.stdout + run.stderr
