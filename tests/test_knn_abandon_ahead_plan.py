"""CPU: the predictor of the abandon checkpoint's head prefetch (csrc/knn_plan.h: knn_ahead_initial / knn_ahead_next /
knn_ahead_speculate, the text the kernel reads too, and the host model knn_ahead_walk) through tests/knn_abandon_ahead_check.cpp, a
stand-alone program built with AddressSanitizer + UBSan and run ONCE: outcome sequences walked against hand-written used / wasted /
bubble counts, which launches prefetch, where their counters live.  And the binding: the new symbol, option, setter, read-back and
config key."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the predictor's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("abandon_ahead") / "knn_abandon_ahead_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "knn_abandon_ahead_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("knn_abandon_ahead_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    return [line.split() for line in run.stdout.splitlines()], run.stdout, run.stderr


def test_the_program_passes_and_the_sanitizers_report_nothing(program):
    _, out, err = program
    assert out.rstrip().endswith("knn_abandon_ahead_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]


def test_the_walks(program):
    """(used, wasted, bubbles) of the sequences the issue names, as the program printed them: every tile leaves; every tile stays;
    strict alternation; a stay at the first tile; a stay at the last; untested tiles in between; a one-tile chunk"""
    walk = {(f[1], int(f[2])): tuple(int(x) for x in f[3:6]) for f in program[0] if f and f[0] == "walk" and len(f) == 6}
    assert walk[("LLLLL", 1)] == (4, 0, 0) and walk[("LLLLL", 0)] == (0, 0, 4)
    assert walk[("SSSSS", 1)] == (0, 1, 1) and walk[("SSSSS", 0)] == (0, 0, 0)
    assert walk[("LSLSL", 1)] == (1, 2, 3) and walk[("SLSLS", 1)] == (0, 2, 4) and walk[("LSLSL", 0)] == (0, 0, 2)
    assert walk[("SLLLL", 1)] == (2, 1, 2) and walk[("LLLLS", 1)] == (4, 0, 0)
    assert walk[("LULUL", 1)] == (2, 0, 0) and walk[("SUULL", 1)] == (0, 1, 2) and walk[("LUSUL", 1)] == (1, 1, 1)
    assert walk[("L", 1)] == walk[("S", 1)] == walk[("U", 1)] == (0, 0, 0)


def test_the_new_symbol_option_setter_and_config_key(program):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import Config, _lib
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import HipFlatIndex, knn_options_from_config
    header = open(os.path.join(ROOT, "include", "radad_hip.h")).read()
    assert re.search(r"\bint\s+radad_knn_last_abandon_ahead\s*\(", header)
    assert "radad_knn_last_abandon_ahead" in _lib.SIGNATURES and len(_lib.SIGNATURES["radad_knn_last_abandon_ahead"][1]) == 3
    assert re.search(r"#define\s+RADAD_KNN_OPT_ABANDON_AHEAD\s+9\b", header) and _lib.KNN_OPT_ABANDON_AHEAD == 9
    assert ["define", "9"] in program[0]
    assert re.search(r"#define\s+RADAD_ABI_VERSION\s+1\b", header)
    assert callable(HipFlatIndex.set_abandon_ahead) and callable(HipFlatIndex.last_abandon_ahead)
    cfg = Config()
    assert cfg.knn_abandon_ahead is None and "abandon_ahead" not in knn_options_from_config(cfg)
    cfg.knn_abandon_ahead = 0
    assert knn_options_from_config(cfg)["abandon_ahead"] == 0
