"""What a flat search launches (radad_knn_last_launch / _last_scan_*) against tests/data/knn_plan_table.json, on fresh stores of
oracle.synth rows: one search per case, every scan kind, both sides of the plan's boundaries that fit a quick test (16383 / 16384
rows, 16 / 17 queries, k + margin 32 / 33, k 128 / 129, dim % 64, the K-split streaming kernel of wide rows) and the handle's four
kernel options.

The table's "observed" section was RECORDED by this file on an MI355X at the commit the table names ("parent"), i.e. before the
host-side planner moved into csrc/knn_plan.h: the cases below assert that the library still launches exactly that.
    RADAD_PLAN_TABLE_RECORD=<commit hash> [RADAD_PLAN_TABLE_OUT=<file>] pytest tests/test_gpu_plan_table.py -m gpu
writes the section instead of asserting it (nothing else reads these variables)."""
import json
import os

import pytest

from oracle import synth

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "knn_plan_table.json")
FIELDS = ("scan_kind", "query_tiles", "db_splits", "block_threads", "scan_launches", "scan_phases")
VARIANTS = {"base": {}, "hi_off": {"hi_plane": 0}, "smallq_hi0": {"smallq_hi": 0}, "wide_min_q1": {"wide_min_q": 1}, "dense0": {"dense": 0}}

# (nq, k): 16 | 17 queries, k + 6 = 32 | 33 (k 26 | 27), the 16-entry lists' k 16 | 17, k 128 | 129, k 1024; 2100 queries at k 27 / 128 on
# 100 000 rows: a tile scan of two phases
PAIRS = ((1, 1), (1, 10), (16, 10), (17, 10), (64, 10), (300, 10), (2100, 10), (16, 16), (16, 17), (16, 26), (16, 27), (17, 26),
         (17, 27), (300, 27), (2100, 27), (300, 128), (2100, 128), (300, 129), (64, 1024))
FEW = ((1, 10), (16, 10), (17, 10), (300, 10), (16, 27), (300, 129))


def key(dim, rows, nq, k, f16, cosine, variant, margin=6):
    """the table's name of a case (the CPU program tests/knn_plan_check.cpp prints the same names)"""
    return f"d{dim}_n{rows}_q{nq}_k{k}_{'f16' if f16 else 'f32'}_{'cos' if cosine else 'l2'}_m{margin}_{variant}"


def gpu_cases():
    """the subset of the table's grid a quick GPU test can build: rows <= 100 000 at dim 64 / 96 / 100, <= 17 000 at dim 1024"""
    out = []
    for rows in (1000, 6144, 6145, 16383, 16384, 16640, 40000, 100000):
        out += [(64, rows, nq, k, False, False, "base") for nq, k in PAIRS]
    out.append((64, 7, 1, 1, False, False, "base"))
    for dim in (96, 100):
        out += [(dim, rows, nq, k, False, False, "base") for rows in (16383, 16384, 100000) for nq, k in FEW]
    for rows in (1000, 6145, 16383, 16384, 16640):
        out += [(1024, rows, nq, k, False, False, "base") for nq, k in FEW + ((16, 16), (16, 17))]
    for rows in (1000, 6144, 16384, 40000):       # (an fp16 store below 16 384 rows: the fp16-operand tile kernel, f16_tile)
        out += [(64, rows, nq, k, True, False, "base") for nq, k in FEW + ((17, 26), (300, 26))]
    for rows in (6144, 16384):
        out += [(64, rows, nq, k, False, True, "base") for nq, k in FEW]
    for variant in ("hi_off", "smallq_hi0", "wide_min_q1", "dense0"):
        out += [(64, rows, nq, 10, False, False, variant) for rows in (6144, 16384) for nq in (1, 16, 17, 300)]
        out += [(1024, 16384, nq, 10, False, False, variant) for nq in (1, 300)]
    return [c for c in out if c[3] <= c[1]]


@pytest.fixture(scope="module")
def pool():
    """one block of synthetic values, cut into [rows, dim] stores and [nq, dim] batches of every shape below"""
    return synth.rows(0, 16640, 1024, 20261).reshape(-1), synth.rows(0, 2100, 1024, 977).reshape(-1)


def observe(case, pool):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    dim, rows, nq, k, f16, cosine, variant = case
    idx = HipFlatIndex(dim, _lib.METRIC_COSINE if cosine else _lib.METRIC_L2, 0, 0, store_f16=f16, **VARIANTS[variant])
    idx.add(pool[0][:rows * dim].reshape(rows, dim))
    idx.search(pool[1][:nq * dim].reshape(nq, dim), k)
    launch = idx.last_launch()
    return [launch[f] for f in FIELDS]


def test_the_subset_covers_what_it_claims():
    cases = gpu_cases()
    assert len(cases) >= 150 and len(set(cases)) == len(cases)
    assert all(rows <= (17000 if dim == 1024 else 100000) for dim, rows, *_ in cases)
    assert {c[6] for c in cases} == set(VARIANTS)
    if not os.environ.get("RADAD_PLAN_TABLE_RECORD"):
        seen = json.load(open(TABLE))["observed"]
        assert set(seen) == {key(*c) for c in cases}
        assert {v[0] for v in seen.values()} == {"f32_tile", "hi_tile", "f32_smallq", "hi_smallq", "f16_tile", "f32_dense"}
        assert any(v[0] == "hi_tile" and v[4] == 2 for v in seen.values())       # a tile scan of two phases


def test_a_search_launches_what_the_table_says(gpu, pool):
    record = os.environ.get("RADAD_PLAN_TABLE_RECORD")
    got = {key(*c): observe(c, pool) for c in gpu_cases()}
    if record:
        out = os.environ.get("RADAD_PLAN_TABLE_OUT", TABLE)
        table = json.load(open(out)) if os.path.exists(out) else {}
        table.update(parent=record, observed_fields=list(FIELDS), observed=got)
        with open(out, "w") as f:
            json.dump(table, f, indent=0, sort_keys=True)
        return
    want = json.load(open(TABLE))["observed"]
    wrong = {name: (row, want[name]) for name, row in got.items() if row != want[name]}
    assert not wrong, f"{len(wrong)} of {len(got)} searches launched something else (got, table): {dict(list(wrong.items())[:8])}"
