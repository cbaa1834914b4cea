"""CPU: the host-only planner of the IVF list-scan search (csrc/ivf_plan.h) through tests/ivf_plan_check.cpp, a stand-alone program built
with AddressSanitizer + UBSan and run ONCE: its own assertions on every plan of its grid (layouts, buffer sizes, task bound, split, the
exact scan's launches, LDS, the refusals) and the anchors computed by hand, and chosen lines against tests/data/ivf_plan_table.json.

    RADAD_PLAN_TABLE_UPDATE=1 pytest tests/test_ivf_plan.py
rewrites the table from the program."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "data", "ivf_plan_table.json")
COLUMNS = ["status", "nprobe", "cmargin", "qcap", "npairs", "T", "group_small", "hi_route", "ccap", "split", "scan_grid", "scan_lds", "cap",
           "refine_lds", "xlds", "nslots", "xgrid", "xlaunches", "group_lds",
           "tasks.cnt", "tasks.cur", "tasks.nt", "tasks.tl", "tasks.tp", "tasks.tc", "tasks.pq", "tasks.ps", "tasks.bytes",
           "qbuf.qh", "qbuf.qscale", "qbuf.qconst", "qbuf.eps", "qbuf.cand_cnt", "qbuf.gbound", "qbuf.fsel", "qbuf.fcount", "qbuf.bytes",
           "ws_a", "ws_b", "part_s", "part_i", "cand_s", "cand_i", "xkey", "xid", "xarrive", "admit"]
GRID = 7 * 4 * 7 * 5 * 6 * 2 * 2      # dim, nlist, nq, k, nprobe, plane, admission bitmap
EXTRAS = 3 * 2 * 2 + 6 * 2 * 2 * 5 * 2 + 2 * 3


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """({case name: [columns]}, number of case lines, the program's whole output, its stderr)"""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("ivf_plan") / "ivf_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "ivf_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("ivf_plan_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, "\n".join(l for l in run.stdout.splitlines() if not l.startswith("case "))[-3000:] + run.stderr[-3000:]
    cases, lines = {}, 0
    for line in run.stdout.splitlines():
        if line.startswith("case "):
            f = line.split()
            row = [int(v) for v in f[2:]]
            assert cases.setdefault(f[1], row) == row      # (nprobe = nlist repeats nprobe 8 at nlist 8: the same plan)
            lines += 1
    return cases, lines, run.stdout, run.stderr


COMMENT = [
    "What an IVF list-scan search launches and allocates (csrc/ivf_plan.h), per case",
    "d<dim>_l<nlist>_q<nq>_k<k>_p<nprobe asked for>_<plane|noplane>_<admit|all>, one case per line, every column ('columns').",
    "A REGRESSION PIN from the commit that moved the plan out of ivf_search_lists on: written by tests/ivf_plan_check.cpp, i.e. by the",
    "new code.  That these are the values the function computed before rests on its expressions having been moved verbatim, on the",
    "anchors tests/ivf_plan_check.cpp asserts (computed by hand from the old expressions) and on the GPU tests.",
    "Cases: the benchmark shape and its one-query form; both sides of nq 16 / 17 (candidate buffers), 128 / 129 at nprobe 32 (one-launch",
    "grouping), nlist 8192 / 8193, k 10 / 11 (16- and 32-entry lists), nprobe 26 / 27 / 32 (coarse margin), the exact scan's launch",
    "boundary 1260 / 1261; dims 512, 5376 and one with one query per task; rows so wide that a search is refused; 2^31 pairs.",
]


def _pinned_names(cases):
    flag = [(p, a) for p in ("plane", "noplane") for a in ("all", "admit")]
    names = [f"d{d}_l{l}_q{q}_k{k}_p{p}_{pl}_all" for d in (512, 5376, 16384) for l in (64, 4096) for q in (1, 16, 17, 1024)
             for k in (10, 11) for p in (26, 27, 32) for pl in ("plane", "noplane")]
    names += [f"d512_l{l}_q{q}_k15_p32_{pl}_{a}" for l in (4096, 8193) for q in (1, 128, 129, 1024) for pl, a in flag]
    names += [f"d64_l{l}_q{q}_k{k}_p{l}_{pl}_admit" for l in (8, 4096, 8193) for q in (1024, 6000) for k in (1, 26) for pl in ("plane", "noplane")]
    names += [n for n in cases if n.startswith("d64_l256_") or n.split("_")[0] in ("d37792", "d37824", "d40000", "d71488", "d71552", "d80000")
              or "_l1048576_" in n]
    assert all(n in cases for n in names)
    return sorted(set(names))


def test_the_program_passes_and_the_sanitizers_report_nothing(program):
    cases, lines, out, err = program
    assert out.rstrip().endswith("ivf_plan_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]
    assert lines == GRID + EXTRAS
    assert all(len(row) == len(COLUMNS) for row in cases.values())
    if os.environ.get("RADAD_PLAN_TABLE_UPDATE"):
        with open(TABLE, "w") as f:
            f.write("{\n" + f'"_comment": [\n' + ",\n".join("  " + json.dumps(c) for c in COMMENT) + "\n],\n")
            f.write(f'"columns": {json.dumps(COLUMNS)},\n"pinned": {{\n')
            f.write(",\n".join(f"  {json.dumps(n)}: {json.dumps(cases[n])}" for n in _pinned_names(cases)) + "\n}\n}\n")


def test_the_plans_are_the_pinned_ones(program):
    cases = program[0]
    table = json.load(open(TABLE))
    assert table["columns"] == COLUMNS and set(table["pinned"]) == set(_pinned_names(cases)) and 300 <= len(table["pinned"]) <= 800
    wrong = {n: [(c, now, was) for c, now, was in zip(COLUMNS, cases[n], row) if now != was] for n, row in table["pinned"].items() if cases[n] != row}
    assert not wrong, f"{len(wrong)} pinned plans changed (column, now, table): {dict(list(wrong.items())[:8])}"


def test_the_pins_hold_the_hand_computed_anchors():
    """the table itself against the values computed by hand from ivf_search_lists as it was (the program asserts the same of the code)"""
    pinned = json.load(open(TABLE))["pinned"]
    col = lambda name, c: pinned[name][COLUMNS.index(c)]
    bench, one = "d512_l4096_q1024_k15_p32_plane_all", "d512_l4096_q1_k15_p32_plane_all"
    want = {"npairs": 32768, "T": 6145, "group_small": 0, "ccap": 2048, "split": 1, "tasks.bytes": 368656, "cap": 512, "refine_lds": 27904,
            "nslots": 1024, "xgrid": 4096, "xlds": 4096, "scan_lds": 37376, "qcap": 16, "cmargin": 0}
    assert {c: col(bench, c) for c in want} == want
    want = {"T": 35, "group_small": 1, "ccap": 8192, "split": 5}
    assert {c: col(one, c) for c in want} == want
    assert col("d512_l4096_q1024_k15_p32_noplane_all", "scan_lds") == 45568
    assert col("d5376_l4096_q1024_k10_p32_plane_all", "scan_lds") == 74576 and col("d5376_l4096_q1024_k10_p32_noplane_all", "scan_lds") == 120144
    assert col("d5376_l4096_q1024_k10_p32_plane_all", "qcap") == 5 and col("d16384_l4096_q1024_k10_p32_plane_all", "qcap") == 1
    assert [col(f"d512_l4096_q1024_k10_p{p}_plane_all", "cmargin") for p in (26, 27, 32)] == [6, 5, 0]
    assert [(col(f"d64_l256_q{q}_k26_p256_plane_all", "nslots"), col(f"d64_l256_q{q}_k26_p256_plane_all", "xlaunches")) for q in (1260, 1261, 1300)] == \
        [(1260, 1), (1260, 2), (1260, 2)]
