"""CPU: the host-only plan of the range calls with RADAD_KNN_OPT_RANGE_SMALLQ (knn_range_plan / knn_range_excl_plan, csrc/knn_plan.h)
through tests/knn_range_smallq_plan_check.cpp, a stand-alone program built with AddressSanitizer + UBSan where the runtimes exist and
run ONCE: with the option 0 every plan is the one in force before it; with the option 1 RADAD_RANGE_STREAM is chosen exactly for
batches of <= 16 queries the plain search could stream the plane for; the stream plan has one 4096-entry buffer per query, one launch
and covers the store; knn_finish_plan's streaming geometry did not move.  And the binding: the two new defines of the header equal the
_lib constants, the ABI version is 1."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """({case: (route, emit_cap, launches, rows_per_wave, n_splits)}, the program's whole output, its stderr)"""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("knn_range_smallq_plan") / "knn_range_smallq_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "knn_range_smallq_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("knn_range_smallq_plan_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    plans = {f[1]: tuple(int(v) for v in f[2:7]) for f in (line.split() for line in run.stdout.splitlines()) if f and f[0] == "plan"}
    return plans, run.stdout, run.stderr


def test_the_program_passes_and_the_sanitizers_report_nothing(program):
    plans, out, err = program
    assert out.rstrip().endswith("knn_range_smallq_plan_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]
    assert len(plans) == 5 * 4 * 5 * 2 * 2 * 2 * 2 * 2


def test_routes_at_named_shapes(program):
    """TILE = 0, EXACT = 1, STREAM = 2"""
    plans = program[0]
    base = dict(n=20480, d=64, q=1, off=0, skip=0, f16=0, sq=1, opt=1)

    def plan(**change):
        c = dict(base, **change)
        return plans[f"n{c['n']}_d{c['d']}_q{c['q']}_off{c['off']}_skip{c['skip']}_f16{c['f16']}_sq{c['sq']}_opt{c['opt']}"]

    def route(**change):
        return plan(**change)[0]
    tile, exact, stream = 0, 1, 2
    assert route() == stream and route(q=16) == stream and route(f16=1) == stream
    assert route(q=17) == tile and route(q=300) == tile
    assert route(n=16383) == exact and route(n=16384) == stream
    assert route(d=96) == exact and route(off=1) == exact and route(skip=8) == exact and route(sq=0) == exact
    assert route(d=5376, q=16) == tile and route(d=5376, q=1) == stream
    for q in (1, 16):                                        # the option off: today's routes
        assert plan(q=q, opt=0) == (exact, 0, 0) + plan(q=q, opt=0)[3:]
    assert plan(q=17, opt=0) == plan(q=17, opt=1)
    r, cap, launches, rpw, splits = plan(n=1000000, d=512)
    assert (r, cap, launches) == (stream, 4096, 1) and splits * 4 * rpw >= 1000000
    for key, p in plans.items():
        if p[0] == stream:
            assert p[1:3] == (4096, 1) and "_opt1" in key and "_off0" in key and "_skip0" in key and "_sq1" in key
        if "_opt0" in key:                                   # the option changes a plan only by choosing the stream
            on = plans[key.replace("_opt0", "_opt1")]
            assert p[0] in (tile, exact) and (on == p or on[0] == stream)


def test_the_new_defines_equal_the_bindings():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    header = open(os.path.join(ROOT, "include", "radad_hip.h")).read()
    opt = re.search(r"#define\s+RADAD_KNN_OPT_RANGE_SMALLQ\s+(\d+)\b", header)
    route = re.search(r"#define\s+RADAD_RANGE_STREAM\s+(\d+)\b", header)
    assert opt and route
    assert int(opt.group(1)) == _lib.KNN_OPT_RANGE_SMALLQ == 6
    assert int(route.group(1)) == _lib.RANGE_STREAM == 2
    assert (_lib.RANGE_TILE, _lib.RANGE_EXACT) == (0, 1)
    assert re.search(r"#define\s+RADAD_ABI_VERSION\s+1\b", header)
    # no new symbol: the option goes through radad_knn_set_option, the route through radad_knn_last_range
    assert "radad_knn_set_option" in _lib.SIGNATURES and "radad_knn_last_range" in _lib.SIGNATURES
    assert not [n for n in _lib.SIGNATURES if "smallq" in n]


def test_the_python_surface_takes_the_option():
    import inspect
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import Config
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import HipFlatIndex, knn_options_from_config
    assert inspect.signature(HipFlatIndex.__init__).parameters["range_smallq"].default is None
    cfg = Config()
    assert "range_smallq" not in knn_options_from_config(cfg)          # None: the library's default (off)
    cfg.update(knn_range_smallq=True)
    assert knn_options_from_config(cfg)["range_smallq"] is True
