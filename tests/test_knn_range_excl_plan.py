"""CPU: the host-only plan of radad_knn_range_search_excl / _excl_pq (knn_range_excl_plan, csrc/knn_plan.h) through
tests/knn_range_excl_plan_check.cpp, a stand-alone program built with AddressSanitizer + UBSan where the runtimes exist and run ONCE:
over the sibling check's grid the route is knn_range_plan's in both modes, the buffers hold 4096 entries, the scan is one launch, the
batch mode carries the biased instantiation and one pre-pass launch, and the per-query mode's plan is knn_range_plan's plan.  And the
binding: both new symbols are declared in the header and bound in _lib.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """({case: (route, emit_cap, launches, biased, prepass)}, the program's whole output, its stderr)"""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("knn_range_excl_plan") / "knn_range_excl_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "knn_range_excl_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("knn_range_excl_plan_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    plans = {f[1]: tuple(int(v) for v in f[2:7]) for f in (line.split() for line in run.stdout.splitlines()) if f and f[0] == "plan"}
    return plans, run.stdout, run.stderr


def test_the_program_passes_and_the_sanitizers_report_nothing(program):
    plans, out, err = program
    assert out.rstrip().endswith("knn_range_excl_plan_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]
    assert len(plans) == 5 * 3 * 5 * 7 * 2 * 2 * 2 * 2


def test_routes_buffers_launches_and_bias_at_named_shapes(program):
    """(route, emit_cap, launches, biased, pre-pass launches); TILE = 0, EXACT = 1; mode 0 = one set for the batch, 1 = per query"""
    plans = program[0]
    base = dict(n=20480, d=64, q=300, m=10, off=0, skip=0, f16=0, mode=0)

    def plan(**change):
        c = dict(base, **change)
        return plans[f"n{c['n']}_d{c['d']}_q{c['q']}_m{c['m']}_off{c['off']}_skip{c['skip']}_f16{c['f16']}_mode{c['mode']}"]
    # (`biased` is the plan's member: the batch mode forces it; the per-query plan leaves it to the caller, who decides it by the
    # plane as for the plain range search)
    assert plan() == (0, 4096, 1, 1, 1) and plan(mode=1) == (0, 4096, 1, 0, 0)
    assert plan(f16=1) == (0, 4096, 1, 1, 1) and plan(q=17, mode=1) == (0, 4096, 1, 0, 0)
    for mode in (0, 1):
        for m in (1, 10, 58, 59, 128, 129, 1024):         # max_per_query does not choose the route
            assert plan(m=m, mode=mode)[:3] == (0, 4096, 1) and plan(m=m, q=16, mode=mode)[:3] == (1, 0, 0)
        for change in (dict(q=16), dict(q=1), dict(n=16383), dict(d=96), dict(off=1), dict(skip=8)):
            assert plan(mode=mode, **change) == (1, 0, 0, 0, 0), change       # exact route: no scan, no bias, no pre-pass
        assert plan(n=16384, mode=mode)[0] == 0 and plan(n=1000000, d=512, q=1024, mode=mode)[:3] == (0, 4096, 1)
    for key, p in plans.items():
        assert p[:3] in ((0, 4096, 1), (1, 0, 0)), key
        assert p[4] == (1 if key.endswith("_mode0") and p[0] == 0 else 0), key


def test_the_new_symbols_are_declared_and_bound():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    header = open(os.path.join(ROOT, "include", "radad_hip.h")).read()
    for name, n_args in (("radad_knn_range_search_excl", 14), ("radad_knn_range_search_excl_pq", 15)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    assert re.search(r"#define\s+RADAD_ABI_VERSION\s+1\b", header)
    assert "exclusion sets combined with a radius;" not in header              # no longer on the not-offered list
