"""CPU: the host side of the tile scan's early abandon (csrc/knn_plan.h) through tests/abandon_plan_check.cpp, a stand-alone program
built with AddressSanitizer + UBSan and run ONCE: the checkpoint for row widths 64 ... 16380, which launches take the ABANDON
instantiation, the layouts.  And the binding: the new symbol, option and config key."""
import os
import re
import shutil
import subprocess

import pytest

import abandon_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("abandon_plan") / "abandon_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "abandon_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("abandon_plan_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    rows = [line.split() for line in run.stdout.splitlines()]
    return rows, run.stdout, run.stderr


def test_the_program_passes_and_the_sanitizers_report_nothing(program):
    rows, out, err = program
    assert out.rstrip().endswith("abandon_plan_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]


def test_checkpoints_agree_with_the_numpy_model(program):
    cps = {int(f[1][1:]): int(f[2]) for f in program[0] if f and f[0] == "checkpoint"}
    assert len(cps) == 254 and min(cps) == 128 and max(cps) == 16320
    for dim, c in cps.items():
        assert c == abandon_ref.checkpoint(dim), dim
    assert cps[128] == 1 and cps[512] == 1 and cps[5376] == 10


def test_which_launches_abandon(program):
    launches = {f[1]: int(f[2]) for f in program[0] if f and f[0] == "launch"}
    assert len(launches) == 2 * 4 * 2 * 2 * 2 * 2 * 2 * 5
    assert launches["o1_r0_s0_k1_f1_b0_c1_d512"] == 1 and launches["o1_r3_s0_k1_f1_b0_c1_d5376"] == 10
    for off in ("o0_r0_s0_k1_f1_b0_c1_d512",      # switched off
                "o1_r1_s0_k1_f1_b0_c1_d512", "o1_r2_s0_k1_f1_b0_c1_d512",      # per-row scales
                "o1_r0_s1_k1_f1_b0_c1_d512",      # the sample pre-pass
                "o1_r0_s0_k2_f1_b0_c1_d512",      # K split
                "o1_r0_s0_k1_f0_b0_c1_d512",      # no floors
                "o1_r0_s0_k1_f1_b1_c1_d512",      # the exclusion scan's per-call bias
                "o1_r0_s0_k1_f1_b0_c0_d512",      # per-tile norms not current
                "o1_r0_s0_k1_f1_b0_c1_d64", "o1_r0_s0_k1_f1_b0_c1_d100"):
        assert launches[off] == 0, off


def test_the_new_symbol_option_and_config_key():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.config import Config
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import knn_options_from_config
    header = open(os.path.join(ROOT, "include", "radad_hip.h")).read()
    assert re.search(r"\bint\s+radad_knn_last_abandon\s*\(", header)
    assert "radad_knn_last_abandon" in _lib.SIGNATURES and len(_lib.SIGNATURES["radad_knn_last_abandon"][1]) == 4
    assert re.search(r"#define\s+RADAD_KNN_OPT_ABANDON\s+5\b", header) and _lib.KNN_OPT_ABANDON == 5
    cfg = Config()
    assert cfg.knn_abandon is None and "abandon" not in knn_options_from_config(cfg)
    cfg.knn_abandon = False
    assert knn_options_from_config(cfg)["abandon"] is False
