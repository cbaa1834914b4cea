"""CPU: the range search among the admissible rows of the probed lists without a GPU -- the float64 reference the GPU tests compare
with (tests/ivf_range_excl_ref.py) against a brute force over the whole store and against the plain reference, ivf_plan_range's two
exclusion parameters through tests/ivf_range_excl_plan_check.cpp (a stand-alone program built with AddressSanitizer + UBSan where the
machine has them), the binding of the two new calls, and every argument error of the new surface that is decided before a device is
touched."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ivf_range_excl_ref as XR
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
    db = _clustered(n, dim, 12, 9201)
    q = _clustered(25, dim, 12, 9203)
    cent = O.kmeans_init(db, nlist)
    assign = O.kmeans_assign(db, cent)
    tags = (np.arange(n) % 8).astype(np.int64)
    return db, q, cent, assign, nlist, tags


def _brute(d64, tags, live_of, radius, M):
    """the filtered range over all rows, written out: per query the admissible rows with d64 < radius, (key, id) order"""
    r = float(np.float32(radius))
    nq = len(d64)
    counts = np.zeros(nq, np.int32)
    ids = np.full((nq, M), -1, np.int64)
    for i in range(nq):
        inside = np.flatnonzero((d64[i] < r) & ~np.isin(tags, live_of(i)))
        counts[i] = len(inside)
        order = inside[np.lexsort((inside, d64[i][inside]))][:M]
        ids[i, :len(order)] = order
    return counts, ids


def test_reference_with_every_list_probed_is_the_filtered_brute_force(store):
    db, q, cent, assign, nlist, tags = store
    d64 = ((db.astype(np.float64)[None] - q.astype(np.float64)[:, None]) ** 2).sum(-1)
    pk = RR.probed_keys(db, assign, cent, q, nlist)
    excl = np.array([1, 3, 4], np.int64)
    rng = np.random.default_rng(9205)
    qtags = rng.integers(0, 8, (len(q), 4)).astype(np.int64)                  # any order, repeats allowed
    counts = np.array([(2, 0, 9, -1, 4)[j % 5] for j in range(len(q))], np.int32)
    for radius in (0.0, float(np.median(d64)), float(np.quantile(d64, 0.02)), np.inf):
        for M in (1, 7, 128):
            got = XR.members_batch(pk, tags, excl, radius, M)
            bc, bi = _brute(d64, tags, lambda i: excl, radius, M)
            np.testing.assert_array_equal(got[0], bc)
            np.testing.assert_array_equal(got[1], bi)
            b = XR.brute_batch(db, q, tags, excl, radius, M)
            np.testing.assert_array_equal(got[0], b[0])
            np.testing.assert_array_equal(got[1], b[1])
            got = XR.members_pq(pk, tags, qtags, counts, radius, M)
            bc, bi = _brute(d64, tags, lambda i: qtags[i, :min(max(int(counts[i]), 0), 4)], radius, M)
            np.testing.assert_array_equal(got[0], bc)
            np.testing.assert_array_equal(got[1], bi)
            b = XR.brute_pq(db, q, tags, qtags, counts, radius, M)
            np.testing.assert_array_equal(got[0], b[0])
            np.testing.assert_array_equal(got[1], b[1])
            have = got[1] >= 0
            assert np.isnan(got[2][~have]).all()
            for i in range(len(q)):                                           # nothing listed carries a tag its query excludes
                live = qtags[i, :min(max(int(counts[i]), 0), 4)]
                assert not np.isin(tags[got[1][i][got[1][i] >= 0]], live).any()


def test_reference_with_nothing_excluded_is_the_plain_reference(store):
    db, q, cent, assign, nlist, tags = store
    pk = RR.probed_keys(db, assign, cent, q, 4)
    radius = RR.radius_between(pk, 0, 30)
    plain = RR.ivf_range(db, assign, cent, q, radius, 4, 128)
    for got in (XR.members_batch(pk, tags, None, radius, 128), XR.members_batch(pk, tags, np.zeros(0, np.int64), radius, 128),
                XR.members_batch(pk, tags, np.array([99, 100]), radius, 128),                     # tags no row has
                XR.members_pq(pk, tags, None, None, radius, 128), XR.members_pq(pk, tags, np.zeros((len(q), 0), np.int64), None, radius, 128),
                XR.members_pq(pk, tags, np.full((len(q), 3), 5, np.int64), np.zeros(len(q), np.int32), radius, 128)):
        for a, b in zip(got, plain):
            np.testing.assert_array_equal(a, b)
    # one set for every query, in any order and with repeats, is the batch-wide set
    S = np.array([6, 2, 2, 5], np.int64)
    a = XR.members_pq(pk, tags, np.tile(S, (len(q), 1)), None, radius, 128)
    b = XR.members_batch(pk, tags, np.unique(S), radius, 128)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert (b[0] < plain[0]).any()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found: the planner's check needs a C++ compiler"
    exe = str(tmp_path_factory.mktemp("ivf_range_excl_plan") / "ivf_range_excl_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, PKG, "csrc"), os.path.join(ROOT, "tests", "ivf_range_excl_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr      # anything else is a real error
        print("ivf_range_excl_plan_check: no sanitizer runtimes on this machine, built WITHOUT -fsanitize=address,undefined")
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout, run.stderr


def test_the_plan_check_passes_and_the_sanitizers_report_nothing(program):
    out, err = program
    assert out.rstrip().endswith("ivf_range_excl_plan_check: ok") and "FAILED" not in out
    assert "runtime error" not in err and "Sanitizer" not in err, err[-3000:]


def test_the_plan_check_covers_the_grid(program):
    out, _ = program
    cases = [line for line in out.splitlines() if line.startswith("case ")]
    seen = set()
    for line in cases:
        f = line.split()
        # case dim D nlist L plane P nq N m M nprobe NP admit A pq_m PQ: status S route R qcap Q scan_lds X pq_lds Y admit_words W
        dim, plane, nq, m, nprobe, admit, pq_m = int(f[2]), int(f[6]), int(f[8]), int(f[10]), int(f[12]), int(f[14]), int(f[16].rstrip(":"))
        status, route, scan_lds, pq_lds, words = int(f[18]), int(f[20]), int(f[24]), int(f[26]), int(f[28])
        seen.add((dim, nq, nprobe, m, pq_m, admit))
        assert status == 0, line
        if not plane or dim % 64:
            assert route == 1 and scan_lds == 0, line
        if plane and dim in (64, 512):
            assert route == 0, line
        if admit and pq_m == 0:
            assert words > 1 and pq_lds == 0, line
        else:
            assert words == 0, line
        assert (pq_lds > 0) == (admit == 1 and pq_m > 0), line
    for dim in (32, 64, 96, 512, 5376):
        for nq in (1, 16, 17, 300, 1024):
            for nprobe in (1, 8, 32):
                for m in (1, 65, 128):
                    for pq_m in (0, 1, 64):
                        for admit in (0, 1):
                            assert (dim, nq, nprobe, m, pq_m, admit) in seen
    tail = re.search(r"cases (\d+) hi (\d+) exact (\d+)", out)
    assert int(tail.group(1)) == len(cases) and int(tail.group(2)) > 0 and int(tail.group(3)) > 0


def test_header_binding_and_constants():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    header = open(os.path.join(ROOT, "include", "radad_hip.h")).read()
    head = (r"\s*\(\s*radad_ivf_t\s+h\s*,\s*const\s+float\s*\*\s*q_dev\s*,\s*int64_t\s+nq\s*,\s*int\s+nprobe\s*,\s*float\s+radius\s*,"
            r"\s*int\s+max_per_query\s*,\s*const\s+int64_t\s*\*\s*row_tags_dev\s*(?:/\*.*?\*/)?\s*,")
    tail = (r"\s*int32_t\s*\*\s*out_count_dev\s*(?:/\*.*?\*/)?\s*,\s*float\s*\*\s*out_dist_dev\s*(?:/\*.*?\*/)?\s*,\s*int64_t\s*\*\s*out_idx_dev\s*(?:/\*.*?\*/)?\s*,"
            r"\s*double\s*\*\s*out_key_dev\s*(?:/\*.*?\*/)?\s*,\s*void\s*\*\s*stream\s*\)\s*;")
    assert re.search(r"\bint\s+radad_ivf_range_search_excl" + head + r"\s*const\s+int64_t\s*\*\s*excl_sorted_dev\s*(?:/\*.*?\*/)?\s*,\s*int64_t\s+n_excl\s*," + tail,
                     header, re.S)
    assert re.search(r"\bint\s+radad_ivf_range_search_excl_pq" + head + r"\s*const\s+int64_t\s*\*\s*q_tags_dev\s*(?:/\*.*?\*/)?\s*,\s*int\s+m\s*,"
                     r"\s*const\s+int32_t\s*\*\s*q_tag_counts_dev\s*(?:/\*.*?\*/)?\s*," + tail, header, re.S)
    assert len(_lib.SIGNATURES["radad_ivf_range_search_excl"][1]) == 14 and len(_lib.SIGNATURES["radad_ivf_range_search_excl_pq"][1]) == 15
    assert len(_lib.SIGNATURES["radad_ivf_range_search"][1]) == 11                # the plain call is what it was
    assert "radad_abi_version" in header and _lib.load().radad_abi_version() == 1
    assert "exclusion sets combined with a radius;" not in header
    # the plain call's doc points to the new calls and keeps what is still missing
    doc = header[header.index("Certified range search over the probed lists"):header.index("#define RADAD_IVF_RANGE_HI")]
    assert "radad_ivf_range_search_excl" in doc and "M > 128, sharded IVF" in doc
    assert "Not offered: exclusion sets combined with a radius" not in doc
    # the per-query form has no pre-pass, and the header says so
    new_doc = header[header.index("Certified range search among the rows of the probed lists"):header.index("int radad_ivf_range_search_excl(")]
    assert "RADAD_IVF_OPT_PQ_FILTER has no effect" in new_doc
    plan_h = open(os.path.join(ROOT, PKG, "csrc", "ivf_plan.h")).read()
    assert re.search(r"ivf_plan_range\(const IvfFacts& s, int64_t nq, int m, int nprobe, bool has_admit = false, int pq_m = 0\)", plan_h)


def test_c_argument_errors_without_gpu():
    """a NULL handle is refused before any device call (the other refusals need a trained index: tests/test_gpu_ivf_range_excl.py)"""
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    lib = _lib.load()
    assert lib.radad_ivf_range_search_excl(None, None, 1, 1, 1.0, 128, None, None, 0, None, None, None, None, None) == _lib.RADAD_EINVAL
    assert lib.radad_ivf_range_search_excl_pq(None, None, 1, 1, 1.0, 128, None, None, 0, None, None, None, None, None, None) == _lib.RADAD_EINVAL


def test_python_value_errors_without_gpu():
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.pipeline import HotPathPipeline
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import HipFlatIndex, HipIVFFlatIndex, VectorDatabase
    idx = object.__new__(HipIVFFlatIndex)                              # (no handle: every refusal below comes before the library is called)
    idx.d, idx.nprobe, idx.device = 64, 1, 0
    q = np.zeros((2, 64), np.float32)
    for m in (0, -1, 129, 1024):
        for name, args in (("range_search_probed_excluding_device", (None, None)), ("range_search_probed_excluding", (None, None)),
                           ("range_search_probed_excluding_per_query_device", (None, None)), ("range_search_probed_excluding_per_query", (None, None))):
            with pytest.raises(ValueError, match="max_per_query"):
                getattr(idx, name)(q, 1.0, *args, max_per_query=m)
    for name in ("range_search_probed_excluding_device", "range_search_probed_excluding", "range_search_probed_excluding_per_query_device",
                 "range_search_probed_excluding_per_query"):
        with pytest.raises(ValueError, match="NaN"):
            getattr(idx, name)(q, float("nan"), None, None)
    # the flat store's names on an IVF index keep refusing
    for name in ("range_search", "range_search_excluding", "range_search_excluding_per_query"):
        with pytest.raises(ValueError, match="flat store's search"):
            getattr(idx, name)(q, 1.0)
    vdb = object.__new__(VectorDatabase)
    vdb.index = None
    for name in ("range_search_probed_excluding_batch", "range_search_probed_excluding_per_query_batch"):
        with pytest.raises(ValueError, match="empty"):
            getattr(vdb, name)(q, 1.0)
    vdb.index = object.__new__(HipFlatIndex)
    with pytest.raises(ValueError, match="a flat store has range_search_excluding_batch"):
        vdb.range_search_probed_excluding_batch(q, 1.0, exclude_tags=[1])
    with pytest.raises(ValueError, match="a flat store has range_search_excluding_per_query_batch"):
        vdb.range_search_probed_excluding_per_query_batch(q, 1.0, query_tags=[[1], [2]])
    pipe = object.__new__(HotPathPipeline)
    pipe.vector_db = vdb
    with pytest.raises(ValueError, match="probed_exclusion needs probed=True"):
        pipe.near_duplicates(q, 1.0, probed_exclusion=True, query_paths=["a.wav", "b.wav"])
    with pytest.raises(ValueError, match="probed_exclusion needs probed=True"):
        pipe.near_duplicates(q, 1.0, probed_exclusion=True, exact_exclusion=True, query_paths=["a.wav", "b.wav"])
    with pytest.raises(ValueError, match="a flat store has range_search_excluding_per_query_batch"):      # a flat store behind probed=True
        pipe.near_duplicates(q, 1.0, probed=True, probed_exclusion=True, query_paths=["a.wav", "b.wav"])
    with pytest.raises(ValueError, match="needs query_paths"):
        pipe.near_duplicates(q, 1.0, probed=True, probed_exclusion=True)
    vdb.index = idx
    with pytest.raises(ValueError, match="exact_exclusion is not offered with probed=True"):
        pipe.near_duplicates(q, 1.0, probed=True, exact_exclusion=True, query_paths=["a.wav", "b.wav"])
    with pytest.raises(ValueError, match="exact_exclusion is not offered with probed=True"):
        pipe.near_duplicates(q, 1.0, probed=True, exact_exclusion=True, probed_exclusion=True, query_paths=["a.wav", "b.wav"])
