"""CPU: the host side of the row tail (csrc/knn_plan.h: knn_defer_rowtail, knn_rowtail_span, knn_rowtail_takes) through
tests/knn_row_tail_plan_check.cpp, a stand-alone program built with AddressSanitizer + UBSan where their runtimes exist and run ONCE:
the grid's shape, that the persistent walk takes every list entry below the count exactly once and none at or past it, the hand-computed
anchors."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("row_tail") / "knn_row_tail_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "knn_row_tail_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("knn_row_tail_plan_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    return [line.split() for line in run.stdout.splitlines()], run.stdout, run.stderr


def test_the_program_passes_and_the_sanitizers_report_nothing(program):
    _, out, err = program
    assert out.rstrip().endswith("knn_row_tail_plan_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]


def test_the_anchors(program):
    """(groups of a full list, workgroups per query tile, rounds), worked out by hand.  The grid is cut for 2 workgroups per CU:
    256 CUs x 2 = 512 workgroups, over the benchmark's 4 query tiles 128 each.
      the benchmark's first launch, 131 072 rows = 512 row tiles:  8192 entries / 16 = 512 groups -> min(128, 512) = 128 x 4 rounds
      its second launch, 868 928 rows = 3395 row tiles:           54 320 entries / 16 = 3395 groups -> 128 x 27 rounds (26 x 128 = 3328)
      20 000 rows = 79 row tiles: 1264 entries = 79 groups -> in eights 80 workgroups (fewer than 512 or 256) x 1 round; over 8 query
      tiles 512 / 8 = 64 workgroups x 2 rounds"""
    anchor = {f[1]: tuple(int(x) for x in f[2:5]) for f in program[0] if f and f[0] == "anchor"}
    assert anchor["bench_launch0"] == (512, 128, 4) and anchor["bench_launch1"] == (3395, 128, 27)
    assert anchor["n20000_q1"] == (79, 80, 1) and anchor["n20000_q2"] == (79, 80, 1) and anchor["n20000_q8"] == (79, 64, 2)
