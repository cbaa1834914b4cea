"""CPU: the range search over the probed lists without a GPU -- the float64 reference the GPU tests compare with
(tests/ivf_range_ref.py) against a brute force and against the top-k oracle, the host-only plan (csrc/ivf_plan.h: ivf_plan_range)
through tests/ivf_range_plan_check.cpp, a stand-alone program built with AddressSanitizer + UBSan where the machine has them, and
every argument error of the new surface that is decided before a device is touched."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ivf_range_ref as RR
from oracle import radad_oracle as O
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "radad_retrievalaugmenteddeepfakeaudiodetection_amd"


def _clustered(n, dim, n_clusters, seed):
    centers = synth.rows(0, n_clusters, dim, seed) * np.float32(3.0)
    which = (np.arange(n) * 7919) % n_clusters
    return (centers[which] + synth.rows(0, n, dim, seed + 1)).astype(np.float32)


@pytest.fixture(scope="module")
def store():
    n, dim, nlist = 3000, 32, 16
    db = _clustered(n, dim, 12, 9101)
    q = _clustered(25, dim, 12, 9103)
    cent = O.kmeans_init(db, nlist)
    assign = O.kmeans_assign(db, cent)
    return db, q, cent, assign, nlist


def test_reference_with_every_list_probed_is_the_brute_force(store):
    db, q, cent, assign, nlist = store
    d64 = ((db.astype(np.float64)[None] - q.astype(np.float64)[:, None]) ** 2).sum(-1)        # [nq, n]
    for radius in (0.0, float(np.median(d64)), float(np.quantile(d64, 0.02)), np.inf):
        for M in (1, 7, 128):
            counts, ids, keys, _ = RR.ivf_range(db, assign, cent, q, radius, nlist, M)
            r = float(np.float32(radius))
            for i in range(len(q)):
                inside = np.flatnonzero(d64[i] < r)
                assert counts[i] == len(inside)
                order = inside[np.lexsort((inside, d64[i][inside]))][:M]
                np.testing.assert_array_equal(ids[i, :len(order)], order)
                np.testing.assert_allclose(keys[i, :len(order)], d64[i][order], rtol=1e-14)
                assert (ids[i, len(order):] == -1).all() and np.isnan(keys[i, len(order):]).all()
            b = RR.brute_range(db, q, radius, M)
            np.testing.assert_array_equal(counts, b[0])
            np.testing.assert_array_equal(ids, b[1])


@pytest.mark.parametrize("nprobe,k", [(1, 5), (4, 15), (16, 26)])
def test_reference_agrees_with_the_topk_oracle_just_above_its_kth_distance(store, nprobe, k):
    """a radius just above the k-th distance of the probed-list top-k holds exactly those k rows (the clustered rows have no ties)"""
    db, q, cent, assign, nlist = store
    od, oi = O.ivf_search(db, assign, cent, q, k + 1, nprobe)
    pk = RR.probed_keys(db, assign, cent, q, nprobe)
    for i in range(len(q)):
        assert np.isfinite(od[i, k])                                   # every query's probed lists hold more than k rows
        radius = RR.radius_between([pk[i]], 0, k)
        assert od[i, k - 1] < float(np.float32(radius)) < od[i, k]
        counts, ids, keys, margin = RR.members([pk[i]], radius, 128)
        assert counts[0] == k and margin[0] > 1e-9
        np.testing.assert_array_equal(ids[0, :k], oi[i, :k])
        np.testing.assert_allclose(keys[0, :k], od[i, :k], rtol=1e-14)
        assert (ids[0, k:] == -1).all()


def test_reference_orders_ties_by_insertion_id_and_is_strict():
    db = np.zeros((6, 4), np.float32)
    db[:, 0] = [1, 2, 1, 1, 3, 2]
    cent = np.zeros((1, 4), np.float32)
    counts, ids, keys, margin = RR.ivf_range(db, np.zeros(6, np.int32), cent, np.zeros((1, 4), np.float32), 4.0, 1, 128)
    assert counts[0] == 3 and list(ids[0, :3]) == [0, 2, 3] and margin[0] == 0.0          # key 4 == radius is NOT a member
    counts, ids, _, _ = RR.ivf_range(db, np.zeros(6, np.int32), cent, np.zeros((1, 4), np.float32), 4.5, 1, 4)
    assert counts[0] == 5 and list(ids[0]) == [0, 2, 3, 1]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("ivf_range_plan") / "ivf_range_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, PKG, "csrc"), os.path.join(ROOT, "tests", "ivf_range_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("ivf_range_plan_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout, run.stderr


def test_the_plan_check_passes_and_the_sanitizers_report_nothing(program):
    out, err = program
    assert out.rstrip().endswith("ivf_range_plan_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]


def test_the_plan_check_covers_the_grid_and_both_routes(program):
    out, _ = program
    cases = [line for line in out.splitlines() if line.startswith("case ")]
    seen = set()
    for line in cases:
        f = line.split()
        seen.add((int(f[2]), int(f[8]), int(f[10])))                   # dim, nq, m
    for dim in (32, 64, 96, 512, 1056, 5376):
        for nq in (1, 16, 17, 1024):
            for m in (1, 128):
                assert (dim, nq, m) in seen
    tail = re.search(r"cases (\d+) hi (\d+) exact (\d+)", out)
    assert int(tail.group(1)) == len(cases) and int(tail.group(2)) > 0 and int(tail.group(3)) > 0
    # without a plane, or at a width that has none, the route is the exact one; with a plane at dim 64 / 512 it is the f16 scan
    for line in cases:
        f = line.split()
        dim, plane, status, route = int(f[2]), int(f[6]), int(f[14]), int(f[16])
        if status == 0 and (not plane or dim % 64):
            assert route == 1, line
        if status == 0 and plane and dim in (64, 512):
            assert route == 0, line


def test_header_binding_and_constants():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    header = open(os.path.join(ROOT, "include", "radad_hip.h")).read()
    assert re.search(r"\bint\s+radad_ivf_range_search\s*\(\s*radad_ivf_t\s+h\s*,\s*const\s+float\s*\*\s*q_dev\s*,\s*int64_t\s+nq\s*,\s*int\s+nprobe\s*,"
                     r"\s*float\s+radius\s*,\s*int\s+max_per_query\s*,", header)
    assert re.search(r"\bint\s+radad_ivf_last_range\s*\(\s*radad_ivf_t\s+h\s*,\s*int64_t\s*\*\s*n_queries\s*,\s*int\s*\*\s*route\s*,\s*int\s*\*\s*n_exact\s*,"
                     r"\s*int\s*\*\s*max_emitted\s*\)", header)
    assert re.search(r"#define\s+RADAD_IVF_RANGE_HI\s+0\b", header) and re.search(r"#define\s+RADAD_IVF_RANGE_EXACT\s+1\b", header)
    assert _lib.IVF_RANGE_ROUTES == ("hi_lists", "exact_lists") and _lib.IVF_MAX_K == 128
    assert len(_lib.SIGNATURES["radad_ivf_range_search"][1]) == 11 and len(_lib.SIGNATURES["radad_ivf_last_range"][1]) == 5
    plan_h = open(os.path.join(ROOT, PKG, "csrc", "ivf_plan.h")).read()
    assert re.search(r"IVF_MAX_K\s*=\s*128\b", plan_h) and re.search(r"IVF_RANGE_CAP\s*=\s*4096\b", plan_h)
    assert "radad_abi_version" in header and _lib.load().radad_abi_version() == 1
    # the flat call no longer lists the IVF index as not offered, and says what is still missing there
    flat_doc = header[header.index("Certified range search: EVERY row"):header.index("#define RADAD_RANGE_TILE")]
    assert "radad_ivf_range_search" in flat_doc and "M > 128" in flat_doc and "; the IVF index;" not in flat_doc


def test_c_argument_errors_without_gpu():
    """a NULL handle is refused before any device call (the other refusals need a trained index: tests/test_gpu_ivf_range.py)"""
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    import ctypes as C
    lib = _lib.load()
    assert lib.radad_ivf_range_search(None, None, 1, 1, 1.0, 128, None, None, None, None, None) == _lib.RADAD_EINVAL
    nq, a, b, c = C.c_int64(7), C.c_int(7), C.c_int(7), C.c_int(7)
    assert lib.radad_ivf_last_range(None, C.byref(nq), C.byref(a), C.byref(b), C.byref(c)) == _lib.RADAD_EINVAL
    assert (nq.value, a.value, b.value, c.value) == (7, 7, 7, 7)


def test_python_value_errors_without_gpu():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.pipeline import HotPathPipeline
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import HipFlatIndex, HipIVFFlatIndex, VectorDatabase
    idx = object.__new__(HipIVFFlatIndex)                              # (no handle: every refusal below comes before the library is called)
    idx.d, idx.nprobe, idx.device = 64, 1, 0
    q = np.zeros((2, 64), np.float32)
    for m in (0, -1, 129, 1024):
        with pytest.raises(ValueError, match="max_per_query"):
            idx.range_search_probed_device(q, 1.0, max_per_query=m)
        with pytest.raises(ValueError, match="max_per_query"):
            idx.range_search_probed(q, 1.0, max_per_query=m)
    with pytest.raises(ValueError, match="NaN"):
        idx.range_search_probed_device(q, float("nan"))
    # the old names on an IVF index keep refusing
    for name in ("range_search", "range_search_excluding", "range_search_excluding_per_query"):
        with pytest.raises(ValueError, match="flat store's search"):
            getattr(idx, name)(q, 1.0)
    assert HipIVFFlatIndex._range_csr is HipFlatIndex._range_csr       # one packing, shared
    vdb = object.__new__(VectorDatabase)
    vdb.index = None
    with pytest.raises(ValueError, match="empty"):
        vdb.range_search_probed_batch(q, 1.0)
    vdb.index = object.__new__(HipFlatIndex)
    with pytest.raises(ValueError, match="range_search_batch"):
        vdb.range_search_probed_batch(q, 1.0)
    vdb.index = idx
    with pytest.raises(ValueError, match="flat and single-handle only"):
        vdb.range_search_batch(q, 1.0)
    pipe = object.__new__(HotPathPipeline)
    pipe.vector_db = vdb
    with pytest.raises(ValueError, match="exact_exclusion is not offered with probed=True"):
        pipe.near_duplicates(q, 1.0, probed=True, exact_exclusion=True, query_paths=["a.wav", "b.wav"])
    vdb.index = object.__new__(HipFlatIndex)
    with pytest.raises(ValueError, match="range_search_batch"):
        pipe.near_duplicates(q, 1.0, probed=True)
    for name in ("range_search_probed_device", "range_search_probed", "last_range"):
        assert callable(getattr(HipIVFFlatIndex, name))
    assert callable(VectorDatabase.range_search_probed_batch)
