"""CPU: the host side of removing rows from a flat store in place (csrc/knn_plan.h: knn_remove_plan, knn_remove_layout,
KnnTuning::rows_removed) through tests/knn_remove_plan_check.cpp, a stand-alone program built with AddressSanitizer + UBSan where the
machine has them and run ONCE.  The program checks every plan's shape and executes its moves on an integer array; this file compares
what it prints with the numpy model (tests/knn_remove_ref.py), executes the model's own plans, and covers the binding and the config
key."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import knn_remove_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 200, 257, 1000, 2049, 3001)
STAGES = (1, 64, 65, 100, 256, 1000)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("knn_remove_plan") / "knn_remove_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "knn_remove_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("knn_remove_plan_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    rows = [line.split() for line in run.stdout.splitlines()]
    return rows, run.stdout, run.stderr


def test_the_program_passes_and_the_sanitizers_report_nothing(program):
    rows, out, err = program
    assert out.rstrip().endswith("knn_remove_plan_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]


def test_every_plan_agrees_with_the_numpy_model(program):
    """slab tiling, which slabs go direct, the launches (kind, rows, destination) and the bytes moved, case by case"""
    cases = {f[1]: [int(x) for x in f[2:]] for f in program[0] if f and f[0] == "case"}
    assert len(cases) == len(SIZES) * len(STAGES) * len(R.PATTERNS) + 1
    seen_direct = seen_grouped = 0
    for n in SIZES:
        for opt in STAGES:
            for pat in R.PATTERNS:
                S = R.stage_rows(2048, opt)
                flags = R.pattern_flags(pat, n, S)
                p = R.plan(n, 2048, flags, opt, l2=True)
                kinds = [l[0] for l in p["launches"]]
                want = [S, p["r0"], p["removed"], len(p["slabs"]), sum(s[4] for s in p["slabs"]), kinds.count(R.GATHER),
                        kinds.count(R.SCATTER), kinds.count(R.DIRECT), p["rows_moved"], p["bytes_moved"], R.checksum(p["launches"])]
                assert cases[f"n{n}_s{opt}_{pat}"] == want, (n, opt, pat)
                seen_direct += kinds.count(R.DIRECT)
                seen_grouped += sum(1 for l in p["launches"] if l[0] == R.DIRECT and l[2] > S)
    assert seen_direct > 100 and seen_grouped > 10       # the cases do reach direct slabs, and launches of several of them
    assert cases["n5000_s0_random30"][0] == R.STAGE_BYTES // 2048 and cases["n5000_s0_random30"][3] == 1


def test_slabs_tile_the_store_and_direct_means_a_stage_of_removed_rows_in_front():
    for n in (1, 64, 65, 257, 3001):
        for opt in (64, 100, 1000):
            S = R.stage_rows(2048, opt)
            for pat in R.PATTERNS:
                flags = R.pattern_flags(pat, n, S)
                p = R.plan(n, 2048, flags, opt)
                if not flags.any():
                    assert p["slabs"] == [] and p["launches"] == []
                    continue
                r0 = int(np.flatnonzero(flags)[0])
                at = r0 // S * S
                for row0, rows, before, kept, direct in p["slabs"]:
                    assert row0 == at and 1 <= rows <= S
                    assert before == int(flags[:row0].sum()) and direct == (before >= S)
                    at += rows
                assert at == n


@pytest.mark.parametrize("pat", R.PATTERNS)
def test_the_model_plan_executed_gives_the_kept_rows(pat):
    """the plan's moves on an integer array reproduce a[keep]; a direct launch never writes at or above its first row (execute())"""
    for n in (1, 2, 64, 65, 129, 257, 1000, 3001):
        for opt in (64, 65, 256):
            S = R.stage_rows(2048, opt)
            flags = R.pattern_flags(pat, n, S)
            a = np.arange(n, dtype=np.int64) + 1000
            got = R.execute(R.plan(n, 2048, flags, opt), flags, a)
            assert np.array_equal(got, a[~flags]), (n, opt, pat)


def test_removal_model():
    keep, omap, removed = R.removal(10, [3, 3, -1, 10, 99, 7, 0], id_base=0)
    assert removed == 3 and list(np.flatnonzero(~keep)) == [0, 3, 7]
    assert list(omap) == [-1, 0, 1, -1, 2, 3, 4, -1, 5, 6]
    keep, omap, removed = R.removal(4, [10 ** 9 + 1, 1, 2, 3], id_base=10 ** 9)
    assert removed == 1 and list(omap) == [10 ** 9, -1, 10 ** 9 + 1, 10 ** 9 + 2]


def test_tuning_after_a_removal(program):
    t = {f[1]: dict(zip(f[2::2], (int(x) for x in f[3::2]))) for f in program[0] if f and f[0] == "tuning"}
    # without a removal: the plane was decided at 1000 rows
    assert t["before_removal"] == {"appended_1000": 0, "appended_1001": 1, "due_1999": 0, "due_2000": 1}
    # plane_decided(..., 1000), rows_removed(600): 700 rows count as appended, the rebuild is due at twice the clamped count
    assert t["removed_to_600"] == {"decided": 600, "appended_600": 0, "appended_700": 1, "due_1199": 0, "due_1200": 1}
    assert t["removed_to_1500"] == {"decided": 1000}
    assert t["replan"] == {"due_601": 1, "due_600": 0}
    assert t["removed_all"] == {"decided": 0, "due_0": 0, "due_1": 1}


def test_layout_defaults(program):
    lay = [f for f in program[0] if f and f[0] == "layout"][0]
    assert int(lay[2]) == (64 << 20) // 2048 and int(lay[4]) == 64


def test_the_new_symbols_option_and_config_key():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.config import Config
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import (HipFlatIndex, HipIVFFlatIndex, VectorDatabase,
                                                                                     knn_options_from_config)
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.pipeline import HotPathPipeline
    header = open(os.path.join(ROOT, "include", "radad_hip.h")).read()
    assert re.search(r"\bint\s+radad_knn_remove_ids\s*\(\s*radad_knn_t\s+h\s*,\s*const\s+int64_t\s*\*\s*ids_dev\s*,\s*int64_t\s+n_ids\s*,"
                     r"\s*int64_t\s*\*\s*old_to_new_dev\s*,\s*int64_t\s*\*\s*n_removed_out\s*,\s*void\s*\*\s*stream\s*\)", header)
    assert re.search(r"\bint\s+radad_knn_remove_ids_host\s*\(\s*radad_knn_t\s+h\s*,\s*const\s+int64_t\s*\*\s*ids_host\s*,\s*int64_t\s+n_ids\s*,"
                     r"\s*int64_t\s*\*\s*n_removed_out\s*\)", header)
    assert len(_lib.SIGNATURES["radad_knn_remove_ids"][1]) == 6 and len(_lib.SIGNATURES["radad_knn_remove_ids_host"][1]) == 4
    assert len(_lib.SIGNATURES["radad_knn_last_remove"][1]) == 3
    assert re.search(r"#define\s+RADAD_KNN_OPT_REMOVE_STAGE_ROWS\s+10\b", header) and _lib.KNN_OPT_REMOVE_STAGE_ROWS == 10
    assert _lib.KNN_REMOVE_MIN_STAGE_ROWS == R.MIN_STAGE_ROWS
    plan_h = open(os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc", "knn_plan.h")).read()
    assert re.search(r"KNN_REMOVE_MIN_STAGE_ROWS\s*=\s*64\b", plan_h)
    lib = _lib.load()
    assert lib.radad_knn_remove_ids(None, None, 0, None, None, None) == _lib.RADAD_EINVAL          # NULL handle, before any device call
    assert lib.radad_knn_remove_ids_host(None, None, 0, None) == _lib.RADAD_EINVAL
    cfg = Config()
    assert cfg.knn_remove_stage_rows is None and "remove_stage_rows" not in knn_options_from_config(cfg)
    cfg.knn_remove_stage_rows = 64
    assert knn_options_from_config(cfg)["remove_stage_rows"] == 64
    for cls, name in ((HipFlatIndex, "remove_ids"), (HipIVFFlatIndex, "remove_ids"), (VectorDatabase, "remove_vectors"),
                      (VectorDatabase, "remove_files"), (HotPathPipeline, "remove_files")):
        assert callable(getattr(cls, name))
