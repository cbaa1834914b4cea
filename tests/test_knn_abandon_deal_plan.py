"""CPU: the host side of the abandoning scan's ticket deal (csrc/knn_plan.h: knn_abandon_deal, knn_deal_ticket) through
tests/knn_abandon_deal_check.cpp, a stand-alone program built with AddressSanitizer + UBSan and run ONCE: every ticket of every slot
for 1 ... 5000 row tiles, which launches are dealt and at what granule.  And the binding: the new symbol, option and setter."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("abandon_deal") / "knn_abandon_deal_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "knn_abandon_deal_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("knn_abandon_deal_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    rows = [line.split() for line in run.stdout.splitlines()]
    return rows, run.stdout, run.stderr


def test_the_program_passes_and_the_sanitizers_report_nothing(program):
    rows, out, err = program
    assert out.rstrip().endswith("knn_abandon_deal_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]
    assert sum(1 for f in rows if f and f[0] == "mapping") >= 3           # granules 1, 2 and 4


def test_the_named_launches(program):
    dec = {f[1]: (int(f[2]), int(f[3]), int(f[4])) for f in program[0] if f and f[0] == "decision"}
    assert len(dec) == 4 * 8 * 5
    # the benchmark on a 256-CU part: 4 query tiles, phases of 512 and 3395 row tiles, 8 resident workgroups per (slot, query tile)
    for tiles in (512, 3395):
        dealt, granule, resident = dec[f"c256_q4_t{tiles}"]
        assert dealt == 1 and resident == 8 and granule >= 1 and -(-tiles // granule) // 8 >= 2 * resident
    # the GPU test's smallest store: 1025 row tiles, one and two query tiles
    assert dec["c256_q1_t1025"][0] == 1 and dec["c256_q2_t1025"][0] == 1
    # the 20 000-row stores of the existing tests (79 row tiles, up to 300 queries) stay static on the parts they run on: a resident
    # workgroup would draw less than two tiles
    for cus in (256, 304):
        for qt in (1, 2):
            assert dec[f"c{cus}_q{qt}_t79"][0] == 0, (cus, qt)


def test_the_new_symbol_option_and_setter():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import HipFlatIndex
    header = open(os.path.join(ROOT, "include", "radad_hip.h")).read()
    assert re.search(r"\bint\s+radad_knn_last_abandon_deal\s*\(", header)
    assert "radad_knn_last_abandon_deal" in _lib.SIGNATURES and len(_lib.SIGNATURES["radad_knn_last_abandon_deal"][1]) == 4
    assert re.search(r"#define\s+RADAD_KNN_OPT_ABANDON_DEAL\s+7\b", header) and _lib.KNN_OPT_ABANDON_DEAL == 7
    assert re.search(r"#define\s+RADAD_ABI_VERSION\s+1\b", header)
    assert callable(HipFlatIndex.set_abandon_deal) and callable(HipFlatIndex.last_abandon_deal)
