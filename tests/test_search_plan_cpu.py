"""The plan of one search sub-batch (arroy_amd/csrc/search_plan.h: what runs, in which grids, and where the scratch lies),
checked on the host: a stand-alone program (tests/search_plan_check.cpp, its own main, no device call) built with
AddressSanitizer and UBSan replays every sub-batch recorded from the search before the plan became one function
(tests/golden/search_plan_cases.txt; est_leaves and the share comparisons are double arithmetic, so no fast-math and no
contraction), walks both scratch layouts of each, and holds wave_descent_wanted and sorted_dedup_kind at their thresholds."""
import os
import subprocess

from conftest import ROOT
from test_index_workspace_cpu import compilers

SRC = os.path.join(ROOT, "tests", "search_plan_check.cpp")
CASES = os.path.join(ROOT, "tests", "golden", "search_plan_cases.txt")


def test_every_sub_batch_is_planned_as_recorded(tmp_path):
    exe = str(tmp_path / "search_plan_check")
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
    assert "every sub-batch planned as recorded" in run.stdout and run.stderr == "", run.stdout + run.stderr
