"""CPU: the host-only scan planner and tuning state (csrc/knn_plan.h) through tests/knn_plan_check.cpp, a stand-alone program built
with AddressSanitizer + UBSan and run ONCE: its own assertions (phases, layouts, the retuning ladder, reports, the look before the
exact pass, the plane), and its table of plans against tests/data/knn_plan_table.json.

    RADAD_PLAN_TABLE_UPDATE=1 pytest tests/test_knn_plan.py
rewrites the table's "pinned" and "groups" sections from the program (never "observed": tests/test_gpu_plan_table.py records that)."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "data", "knn_plan_table.json")
COLUMNS = ["scan_kind", "query_tiles", "db_splits", "block_threads", "scan_launches", "scan_phases", "ksel", "ksel_sq", "sq_ksplit",
           "s_splits", "emit_cap", "cap", "plen", "n_parts", "xgroup", "layout_bytes"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """(lines of the program's table: {case name: [columns]}, its whole output, its stderr)"""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("knn_plan") / "knn_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "radad_retrievalaugmenteddeepfakeaudiodetection_amd", "csrc"),
           os.path.join(ROOT, "tests", "knn_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("knn_plan_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    cases = {}
    for line in run.stdout.splitlines():
        if line.startswith("case "):
            f = line.split()
            cases[f[1]] = [f[2]] + [int(v) for v in f[3:]]
    return cases, run.stdout, run.stderr


COMMENT = [
    "What a flat search launches and allocates, per case d<dim>_n<rows>_q<nq>_k<k>_<store>_<metric>_m<margin>_<variant>.",
    "observed: the six fields radad_knn_last_launch / _last_scan_* reported on an MI355X AT THE COMMIT 'parent', i.e. before the",
    "planner moved into csrc/knn_plan.h, recorded by tests/test_gpu_plan_table.py.  They are the parent's behaviour: the planner",
    "(tests/test_knn_plan.py, no GPU) and the library (tests/test_gpu_plan_table.py) are both held to them.",
    "pinned, groups: written by tests/knn_plan_check.cpp, i.e. by the NEW code -- every column ('columns') of the observed cases and of a",
    "few that no quick GPU test reaches (1 M / 1.3 M / 10 M rows, margin 0), and a SHA-256 prefix per (dim, rows, store, metric, margin, variant) over the program's lines",
    "for its 54 (nq, k) cases (the whole grid is 45 630 lines: too large to commit).  Beyond the observed fields these are a regression",
    "pin from that commit on, not proof of equality with the parent: that rests on the functions having been moved verbatim.",
]


def _write(table):
    table["_comment"] = COMMENT
    with open(TABLE, "w") as f:
        f.write("{\n")
        keys = sorted(table)
        for i, key in enumerate(keys):
            v = table[key]
            if isinstance(v, dict):
                body = ",\n".join(f"  {json.dumps(n)}: {json.dumps(v[n])}" for n in sorted(v))
                f.write(f"{json.dumps(key)}: {{\n{body}\n}}")
            elif key == "_comment":
                f.write(f"{json.dumps(key)}: [\n" + ",\n".join("  " + json.dumps(line) for line in v) + "\n]")
            else:
                f.write(f"{json.dumps(key)}: {json.dumps(v)}")
            f.write(",\n" if i + 1 < len(keys) else "\n")
        f.write("}\n")


def _group(name):
    d, n, q, k, rest = name.split("_", 4)
    return f"{d}_{n}_{rest}"


def _digests(cases):
    """one digest per (dim, rows, store, metric, margin, variant): its 54 (nq, k) lines in the program's order"""
    h = {}
    for name, row in cases.items():
        h.setdefault(_group(name), hashlib.sha256()).update((name + " " + " ".join(map(str, row)) + "\n").encode())
    return {g: d.hexdigest()[:16] for g, d in h.items()}


def _pinned_names(cases, table):
    """every recorded case, and what no quick GPU test reaches: the phase boundary at 1.2 M rows and a 10 M-row store (narrow and wide
    rows; fp32, fp16 and widened buffers) and the coarse quantiser's margin 0 on both sides of k + margin = 32"""
    big = [f"d{d}_n{n}_q{q}_k{k}_{v}" for d in (64, 5376) for n in (1000000, 1300000, 10000000)
           for q, k in ((1, 10), (17, 10), (300, 10), (2100, 10), (2100, 128), (300, 129))
           for v in ("f32_l2_m6_base", "f16_l2_m6_base", "f32_l2_m6_cap_boost4")]
    m0 = [f"d64_n{n}_q{q}_k{k}_f32_l2_m0_base" for n in (6144, 16384) for q in (16, 300) for k in (26, 27)]
    assert all(n in cases for n in big + m0)
    return sorted(set(table.get("observed", {})) | set(big) | set(m0))


def test_the_program_passes_and_the_sanitizers_report_nothing(program):
    cases, out, err = program
    assert out.rstrip().endswith("knn_plan_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]
    assert len(cases) == 5 * 13 * 6 * 9 * (2 * 2 * 2 + 5)
    assert all(len(row) == len(COLUMNS) for row in cases.values())
    if os.environ.get("RADAD_PLAN_TABLE_UPDATE"):
        table = json.load(open(TABLE))
        table["columns"] = COLUMNS
        table["pinned"] = {n: cases[n] for n in _pinned_names(cases, table)}
        table["groups"] = _digests(cases)
        _write(table)


def test_the_plans_are_what_the_parent_launched_on_a_gpu(program):
    """the six observable columns of every case tests/test_gpu_plan_table.py recorded at the table's "parent" commit"""
    cases = program[0]
    table = json.load(open(TABLE))
    assert table["observed_fields"] == COLUMNS[:6] and len(table["observed"]) >= 150
    wrong = {n: (cases[n][:6], seen) for n, seen in table["observed"].items() if cases[n][:6] != seen}
    assert not wrong, f"{len(wrong)} plans differ from what the parent launched (planned, recorded): {dict(list(wrong.items())[:8])}"


def test_the_plans_are_the_pinned_ones(program):
    """every column of the pinned cases (all recorded ones, and large stores), and a digest of every group of the whole grid"""
    cases = program[0]
    table = json.load(open(TABLE))
    assert table["columns"] == COLUMNS and set(table["pinned"]) == set(_pinned_names(cases, table))
    wrong = {n: (cases[n], row) for n, row in table["pinned"].items() if cases[n] != row}
    assert not wrong, f"{len(wrong)} pinned plans changed (now, table): {dict(list(wrong.items())[:8])}"
    now = _digests(cases)
    assert set(now) == set(table["groups"])
    changed = sorted(g for g in now if now[g] != table["groups"][g])
    assert not changed, f"{len(changed)} groups of the grid changed, e.g. {changed[:8]}: " + \
        "; ".join(f"{n} {cases[n]}" for n in list(cases) if _group(n) == changed[0])[:3000]
