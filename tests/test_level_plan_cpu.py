"""The per-level plan of the forest build (arroy_amd/csrc/level_plan.h: margin mode, row-major launches, the tail in groups),
checked on the host: a stand-alone program (tests/level_plan_check.cpp, its own main, no device call) built with
AddressSanitizer and UBSan holds tail_group_width against its table, replays every level recorded from the build before the
plan became one function (tests/golden/level_plan_cases.txt; best_cost to the last bit, so no fast-math and no contraction)
and walks the uniform 10M x 768 x 100-tree ladder of DESIGN.md."""
import os
import subprocess

from conftest import ROOT
from test_index_workspace_cpu import compilers

SRC = os.path.join(ROOT, "tests", "level_plan_check.cpp")
CASES = os.path.join(ROOT, "tests", "golden", "level_plan_cases.txt")


def test_every_level_is_planned_as_recorded(tmp_path):
    exe = str(tmp_path / "level_plan_check")
    tried = []
    for cxx in compilers():
        build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all", "-pthread", SRC, "-o", exe], capture_output=True, text=True)
        if build.returncode == 0:
            break
        tried.append(f"{cxx}: {build.stderr[-2000:]}")
    else:
        raise AssertionError("no host compiler built the sanitized program:\n" + "\n".join(tried))
    run = subprocess.run([exe, CASES], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every level planned as recorded" in run.stdout and run.stderr == "", run.stdout + run.stderr
