"""The exclusion-aware IVF search (radad_ivf_search_excl, HipIVFFlatIndex.search_probed_excluding): for every query the exact top-k
among the rows of its probed lists whose tag is not excluded, through every scan route of tests/test_gpu_ivf_adversarial.py

  default   certified f16 list scan, k_ivf_scan_hi<true>; rejected queries take k_ivf_exact<true>
  f32       hi_scan=0: k_ivf_scan<KSEL, true> behind its certificate
  rejected  hi_scan=2: k_ivf_exact<true> answers every query
  noplane   dim 96: the fp32 list scan by itself

The expected answer is the existing oracle on the ADMISSIBLE rows: O.ivf_search(db[adm], assign[adm], ...) with the ids mapped back
through keep = flatnonzero(adm) (monotone: ties still go to the lower id).  ids must be equal, distances agree to rtol 1e-6 / atol
1e-5, unfilled slots hold -1 / NaN.  What makes "ids are equal" a fair demand, and what makes each case the case it claims to be, is
asserted without a GPU by test_cpu_conditions_of_the_cases."""
import os

import numpy as np
import pytest

from oracle import radad_oracle as O
from oracle import synth
from test_gpu_ivf_adversarial import KS, NQS, STORES, _assert_route, _blobs, _index, assert_gaps, cpu_assign, prepared

ROUTES = (("default", 128), ("f32", 128), ("rejected", 128), ("noplane", 96))
KMAX = max(KS)
_CASES = {}


# ---- CPU side -----------------------------------------------------------------------------------------------------------------------
def expected(db, assign, cent, q, k, nprobe, tags, excl, what=""):
    """(float64 distances, ids) [nq, k + 1] of the oracle on the admissible rows, the gap conditions asserted on that filtered store"""
    adm = ~np.isin(tags, excl)
    keep = np.flatnonzero(adm)
    if len(keep) == 0:
        return np.full((len(q), k + 1), np.inf), np.full((len(q), k + 1), -1, np.int64)
    od, oi = assert_gaps(db[adm], assign[adm], cent, q, k, nprobe, what=what)
    return od, np.where(oi >= 0, keep[np.clip(oi, 0, None)], -1)


def _base(dim, n=6000, nlist=24, seed=9901, nq=300):
    cent, db = _blobs(n, dim, nlist, seed)
    q = (cent[(np.arange(nq) * 5) % nlist] + synth.rows(0, nq, dim, seed + 4)).astype(np.float32)
    return db, cent, q


def case_crowded(dim):
    """20 near-copies of each of the queries 3 .. 10 (inside every batch the tests take) stored under excluded tags"""
    rng = np.random.default_rng(9911 + dim)
    db, cent, q = _base(dim)
    tags = np.arange(len(db), dtype=np.int64)
    planted = np.arange(3, 11)
    at = rng.choice(len(db), 8 * 20, replace=False).reshape(8, 20)
    for j, rows in zip(planted, at):
        db[rows] = q[j] + np.float32(1e-3) * rng.standard_normal((20, dim)).astype(np.float32)
        tags[rows] = 1_000_000 + j
    excl = np.sort(np.concatenate([1_000_000 + planted, [2_000_000, -5]])).astype(np.int64)    # (two tags no row has, too)
    return dict(db=db, cent=cent, q=q, tags=tags, excl=excl, nprobe=3, planted=planted)


def case_mostly(dim):
    """about 95 % of the rows excluded (the training_file_ids shape); the lists 0 .. 3 keep no row, list 4 keeps three"""
    rng = np.random.default_rng(9921 + dim)
    db, cent, q = _base(dim, seed=9925)
    assign = cpu_assign(db, cent)
    adm = (rng.random(len(db)) < 0.06) & (assign >= 4)
    r4 = np.flatnonzero(assign == 4)
    adm[r4] = False
    adm[r4[[5, 70, 200]]] = True
    tags = 7 * np.arange(len(db), dtype=np.int64) + 3
    excl = np.sort(tags[~adm])
    return dict(db=db, cent=cent, q=q, tags=tags, excl=excl, nprobe=1, assign=assign)


def case_long_lists(dim):
    """lists longer than 256 rows and one query: every list is split over several workgroups, whose shares start anywhere"""
    rng = np.random.default_rng(9931 + dim)
    db, cent, q = _base(dim, n=30000, nlist=8, seed=9935, nq=17)
    tags = np.arange(len(db), dtype=np.int64)
    ranges = np.concatenate([np.arange(1000, 1130), np.arange(5000, 9001), np.arange(20001, 20064), np.arange(29990, 30000)])
    half = np.flatnonzero(rng.random(len(db)) < 0.5)
    return dict(db=db, cent=cent, q=q, tags=tags, excl=np.sort(ranges), excl2=np.sort(half), nprobe=3)


def case(name, dim):
    """the inputs of a case and its expected answers for k = 26 (every smaller k is a prefix), all conditions asserted"""
    key = (name, dim)
    if key in _CASES:
        return _CASES[key]
    c = {"crowded": case_crowded, "mostly": case_mostly, "long_lists": case_long_lists}[name](dim)
    db, cent, q, tags, excl, nprobe = c["db"], c["cent"], c["q"], c["tags"], c["excl"], c["nprobe"]
    assign = c["assign"] = c.get("assign", cpu_assign(db, cent))
    what = f"{name} dim {dim}"
    c["od"], c["oi"] = expected(db, assign, cent, q, KMAX, nprobe, tags, excl, what)
    if name == "crowded":
        c["plain"] = assert_gaps(db, assign, cent, q, KMAX, nprobe, what=what + " unfiltered")
        for k in KS:       # the reference's loop (search K + 10, drop, pad) is defeated for every planted query
            _, pi = O.ivf_search(db, assign, cent, q[c["planted"]], k + 10, nprobe)
            left = ((pi >= 0) & ~np.isin(tags[np.clip(pi, 0, None)], excl)).sum(1)
            assert np.all(left < k), (what, k, left)
            assert np.all(c["oi"][c["planted"], :k] >= 0), (what, k)                  # ... although k admissible neighbours exist
        # whole-list: every row of query 3's home list excluded
        home = int(O.knn(cent, q[3:4], 1, "L2")[1][0, 0])
        c["home_excl"] = np.sort(tags[assign == home])
        for npb in (1, 3):
            c[f"home{npb}"] = expected(db, assign, cent, q[:40], 15, npb, tags, c["home_excl"], what + f" home list excluded, nprobe {npb}")
        assert np.all(c["home1"][1][3] == -1) and np.all(c["home3"][1][3, :15] >= 0), what
    if name == "mostly":
        assert 0.93 < np.isin(tags, excl).mean() < 0.97, what
        filled = (c["oi"][:, :KMAX] >= 0).sum(1)
        assert (filled == 0).any() and ((filled > 0) & (filled < 15)).any() and (filled == 3).any(), (what, np.bincount(filled))
        c["filled"] = filled
    if name == "long_lists":
        assert np.bincount(assign).min() > 256, what
        c["od2"], c["oi2"] = expected(db, assign, cent, q, KMAX, nprobe, tags, c["excl2"], what + " random half")
    _CASES[key] = c
    return c


def adversarial_case(name):
    """a store of tests/test_gpu_ivf_adversarial.py at dim 128, tags = row ids, the union of the oracle's top-3 ids over the queries
    excluded; the duplicates store also loses half of each duplicate group"""
    key = ("adv", name)
    if key not in _CASES:
        db, q, cent, nprobe, extra, assign, od, oi = prepared(name, 128)
        tags = np.arange(len(db), dtype=np.int64)
        ex = oi[:, :3].ravel()
        ex = ex[ex >= 0]
        if "dups" in extra:
            ex = np.concatenate([ex] + [rows[::2] for rows in extra["dups"].values()])
        excl = np.unique(ex).astype(np.int64)
        eod, eoi = expected(db, assign, cent, q, KMAX, nprobe, tags, excl, f"{name} minus the top-3")
        assert not np.isin(eoi, excl).any()
        _CASES[key] = (db, q, cent, nprobe, extra, assign, tags, excl, eod, eoi)
    return _CASES[key]


@pytest.mark.parametrize("dim", [128, 96])
@pytest.mark.parametrize("name", ["crowded", "mostly", "long_lists"])
def test_cpu_conditions_of_the_cases(name, dim):
    case(name, dim)


@pytest.mark.parametrize("name", list(STORES))
def test_cpu_conditions_of_the_adversarial_cases(name):
    db, q, cent, nprobe, extra, assign, tags, excl, eod, eoi = adversarial_case(name)
    if "dups" in extra:
        for j, rows in extra["dups"].items():
            left = rows[~np.isin(rows, excl)]
            assert len(left) >= 15 and list(eoi[j, :15]) == list(left[:15]), (name, j)


def test_the_library_offers_the_search():
    """no GPU: the symbol is declared, bound and exported (fails on a build without the feature)"""
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    assert "radad_ivf_search_excl" in _lib.SIGNATURES
    assert hasattr(R.HipIVFFlatIndex, "search_probed_excluding") and hasattr(R.VectorDatabase, "search_probed_excluding")
    assert R.Config().ivf_exact_exclusion is False
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "radad_hip.h")).read()
    assert "radad_ivf_search_excl(" in hdr and "Not offered for the IVF index" not in hdr


# ---- GPU side -----------------------------------------------------------------------------------------------------------------------
def _build(gpu, dim, cent, db, route, nprobe):
    idx = _index(gpu, dim, len(cent), route)
    idx.set_centroids(cent)
    half = len(db) // 2
    idx.add(db[:half]); idx.add(db[half:])
    idx.nprobe = nprobe
    return idx


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _search(idx, gpu, q, k, tags, excl):
    D, I = idx.search_probed_excluding(_dev(gpu, q), k, None if tags is None else _dev(gpu, tags), None if excl is None else _dev(gpu, excl))
    return D.cpu().numpy(), I.cpu().numpy()


def _compare(D, I, od, oi, k, excl, what):
    od, oi = od[:, :k], oi[:, :k]
    assert D.shape == oi.shape and I.shape == oi.shape, what
    if excl is not None and len(excl):
        assert not np.isin(I, excl).any(), f"{what}: an excluded id was returned"      # (tags are the ids in the cases that pass excl)
    bad = np.flatnonzero((I != oi).any(1))
    assert len(bad) == 0, f"{what}: ids differ from the oracle for {len(bad)} of {len(I)} queries, first {bad[:5]}: {I[bad[0]]} vs {oi[bad[0]]}"
    fin = oi >= 0
    np.testing.assert_allclose(D[fin], od[fin], rtol=1e-6, atol=1e-5, err_msg=str(what))
    assert np.all(np.isnan(D[~fin])) and np.all(I[~fin] == -1), what


def _sweep(idx, gpu, route, q, tags, excl, od, oi, what, nqs=NQS, ks=KS, ids_are_tags=False):
    failures = []
    for nq in nqs:
        sl = slice(3, 3 + nq) if nq < len(q) else slice(0, len(q))
        for k in ks:
            w = dict(what=what, route=route, nq=nq, k=k)
            D, I = _search(idx, gpu, q[sl], k, tags, excl)
            info = idx.last_search_info()
            try:
                _compare(D, I, od[sl], oi[sl], k, excl if ids_are_tags else None, w)
                _assert_route(info, route, len(q[sl]), w)
            except (AssertionError, KeyError) as e:
                failures.append(f"{w} {info}: {str(e)[:300]}")
    assert not failures, f"{len(failures)} searches wrong:\n" + "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("route,dim", ROUTES)
def test_nothing_excluded_is_the_plain_search(gpu, route, dim):
    """NULL / n_excl == 0, and a set that shares no tag with the store: ids and filled distances bit-equal to idx.search"""
    c = case("crowded", dim)
    idx = _build(gpu, dim, c["cent"], c["db"], route, c["nprobe"])
    none = np.array([-7, 1_500_000, 3_000_000], np.int64)
    assert not np.isin(c["tags"], none).any()
    for nq in NQS:
        sl = slice(3, 3 + nq) if nq < 300 else slice(0, 300)
        for k in KS:
            D0, I0 = idx.search(c["q"][sl], k)
            for tags, excl in ((None, None), (c["tags"], np.zeros(0, np.int64)), (c["tags"], none)):
                D, I = _search(idx, gpu, c["q"][sl], k, tags, excl)
                _assert_route(idx.last_search_info(), route, len(I), (route, nq, k))
                fin = I0 >= 0
                assert np.array_equal(I, I0) and np.array_equal(D[fin], D0[fin]) and np.all(np.isnan(D[~fin])), (route, nq, k)
            _compare(D, I, c["plain"][0][sl], c["plain"][1][sl], k, None, (route, nq, k))


@pytest.mark.gpu
@pytest.mark.parametrize("route,dim", ROUTES)
def test_crowded_queries_get_real_neighbours(gpu, route, dim):
    c = case("crowded", dim)
    idx = _build(gpu, dim, c["cent"], c["db"], route, c["nprobe"])
    _sweep(idx, gpu, route, c["q"], c["tags"], c["excl"], c["od"], c["oi"], "crowded")
    D, I = _search(idx, gpu, c["q"], 15, c["tags"], c["excl"])
    assert np.all(I[c["planted"]] >= 0) and not np.isin(c["tags"][I[c["planted"]]], c["excl"]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("route,dim", ROUTES)
def test_mostly_excluded_store(gpu, route, dim):
    """the exact counts of filled slots, and no excluded row in any slot (what a score of -inf alone does not give)"""
    c = case("mostly", dim)
    idx = _build(gpu, dim, c["cent"], c["db"], route, c["nprobe"])
    _sweep(idx, gpu, route, c["q"], c["tags"], c["excl"], c["od"], c["oi"], "mostly excluded")
    D, I = _search(idx, gpu, c["q"], KMAX, c["tags"], c["excl"])
    assert np.array_equal((I >= 0).sum(1), c["filled"])
    assert not np.isin(c["tags"][I[I >= 0]], c["excl"]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("route,dim", ROUTES)
def test_whole_list_and_everything_excluded(gpu, route, dim):
    c = case("crowded", dim)
    idx = _build(gpu, dim, c["cent"], c["db"], route, 1)
    q = c["q"][:40]
    for npb in (1, 3):
        idx.nprobe = npb
        D, I = _search(idx, gpu, q, 15, c["tags"], c["home_excl"])
        _compare(D, I, *c[f"home{npb}"], 15, None, (route, "home list excluded", npb))
        _assert_route(idx.last_search_info(), route, 40, (route, npb))
    assert np.all(I[3] >= 0)
    D, I = _search(idx, gpu, q, 5, c["tags"], np.unique(c["tags"]))
    assert np.all(I == -1) and np.all(np.isnan(D))
    _assert_route(idx.last_search_info(), route, 40, (route, "all excluded"))


@pytest.mark.gpu
@pytest.mark.parametrize("route,dim", ROUTES)
def test_bit_indexing_in_split_lists(gpu, route, dim):
    """The f16 routes split a list over `split` workgroups when a search has few tasks (radad_ivf_search_excl's host code: T <= 64
    gives 8, capped by (cand_cap / 2) / (nprobe (k + 8))).  Here nprobe = 3 and 8 lists: one query has T = 3 + 0 + 1 = 4 tasks (bound) and
    the cap is 4096 / (3 * 34) = 40; 17 queries have T = 8 + 51 / 16 + 1 = 12 and the cap is 1024 / 102 = 10 -- split = 8 both times, so
    a workgroup's share of a ~3750-row list is 480 rows and starts at l_begin + 480 sub, on no multiple of 64 in general.  If that
    heuristic changes, choose nq / nprobe here so that split stays above 1."""
    c = case("long_lists", dim)
    idx = _build(gpu, dim, c["cent"], c["db"], route, c["nprobe"])
    _sweep(idx, gpu, route, c["q"], c["tags"], c["excl"], c["od"], c["oi"], "ranges", nqs=(1, 17), ks=(5, 26), ids_are_tags=True)
    _sweep(idx, gpu, route, c["q"], c["tags"], c["excl2"], c["od2"], c["oi2"], "random half", nqs=(1, 17), ks=(1, 15), ids_are_tags=True)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["default", "f32", "rejected"])
@pytest.mark.parametrize("name", list(STORES))
def test_adversarial_stores_minus_their_top3(gpu, name, route):
    db, q, cent, nprobe, extra, assign, tags, excl, eod, eoi = adversarial_case(name)
    idx = _build(gpu, 128, cent, db, route, nprobe)
    np.testing.assert_array_equal(idx.assignments(), assign)
    _sweep(idx, gpu, route, q, tags, excl, eod, eoi, name, ids_are_tags=True)
    if "dups" in extra:                                   # exact ties among the survivors: the lowest ids first
        D, I = _search(idx, gpu, q, 15, tags, excl)
        for j, rows in extra["dups"].items():
            left = rows[~np.isin(rows, excl)]         # (half of the group, and whatever the top-3 of the queries took)
            assert list(I[j]) == list(left[:15]), (j, I[j])


@pytest.mark.gpu
@pytest.mark.parametrize("route,dim", ROUTES)
def test_add_between_searches_and_two_streams(gpu, route, dim):
    import torch
    c = case("crowded", dim)
    db, cent, q, tags, excl = c["db"], c["cent"], c["q"][:40], c["tags"], c["excl"]
    idx = _build(gpu, dim, cent, db, route, 3)
    D0, I0 = _search(idx, gpu, q, 5, tags, excl)
    _compare(D0, I0, c["od"][:40], c["oi"][:40], 5, None, "before the append")
    # eight admissible rows 2e-3 from the queries 20 .. 27, eight excluded ones 1e-3 from them
    good = (q[20:28] + np.float32(2e-3) * synth.rows(0, 8, dim, 9941)).astype(np.float32)
    evil = (q[20:28] + np.float32(1e-3) * synth.rows(8, 8, dim, 9941)).astype(np.float32)
    idx.add(good); idx.add(evil)
    db2 = np.concatenate([db, good, evil])
    tags2 = np.concatenate([tags, 3_000_000 + np.arange(8), np.full(8, 1_000_003)]).astype(np.int64)
    assert 1_000_003 in excl
    od, oi = expected(db2, idx.assignments(), cent, q, 5, 3, tags2, excl, "after the append")
    D1, I1 = _search(idx, gpu, q, 5, tags2, excl)
    _compare(D1, I1, od, oi, 5, None, "after the append")
    _assert_route(idx.last_search_info(), route, 40, route)
    assert np.array_equal(I1[20:28, 0], len(db) + np.arange(8)) and not (I1 >= len(db) + 8).any()
    with pytest.raises(ValueError, match="one tag per stored row"):
        idx.search_probed_excluding(_dev(gpu, q), 5, _dev(gpu, tags), _dev(gpu, excl))
    # the same search on two streams alternately
    s = [torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)]
    qd, td, ed = _dev(gpu, q), _dev(gpu, tags2), _dev(gpu, excl)
    torch.cuda.synchronize()
    outs = []
    for it in range(6):
        with torch.cuda.stream(s[it % 2]):
            outs.append(idx.search_probed_excluding(qd, 5, td, ed))
    torch.cuda.synchronize()
    for Dd, Id in outs:
        assert np.array_equal(Id.cpu().numpy(), I1) and np.array_equal(Dd.cpu().numpy(), D1, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("route,dim", ROUTES)
def test_arguments(gpu, route, dim):
    c = case("crowded", dim)
    q, tags, excl = c["q"][:4], c["tags"], c["excl"]
    idx = _index(gpu, dim, len(c["cent"]), route)
    with pytest.raises(ValueError, match="not trained"):
        _search(idx, gpu, q, 5, None, None)
    idx.set_centroids(c["cent"])
    idx.nprobe = 3
    D, I = _search(idx, gpu, q, 5, None, None)                          # a trained index without rows
    assert np.all(I == -1) and np.all(np.isnan(D))
    idx.add(c["db"])
    with pytest.raises(ValueError, match="26"):
        _search(idx, gpu, q, 27, tags, excl)
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    import torch
    qd = _dev(gpu, q)
    D = torch.empty((4, 27), device=gpu); I = torch.empty((4, 27), device=gpu, dtype=torch.int64)
    rc = idx._lib.radad_ivf_search_excl(idx._h, qd.data_ptr(), 4, 27, 3, None, None, 0, D.data_ptr(), I.data_ptr(), _lib.stream_ptr(qd.device))
    assert rc == _lib.RADAD_EINVAL and b"26" in idx._lib.radad_last_error()
    rc = idx._lib.radad_ivf_search_excl(idx._h, qd.data_ptr(), 4, 5, 3, None, None, 2, D.data_ptr(), I.data_ptr(), _lib.stream_ptr(qd.device))
    assert rc == _lib.RADAD_EINVAL
    with pytest.raises(ValueError, match="one tag per stored row"):
        _search(idx, gpu, q, 5, tags[:-1], excl)
    D, I = _search(idx, gpu, q, 5, tags, excl)
    _compare(D, I, c["od"][:4], c["oi"][:4], 5, None, "after the refusals")
    assert idx.last_search_info()["scan"] != "exact_flat"


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipeline_ivf_exact_exclusion(gpu, tmp_path):
    """the crowded store of tests/test_gpu_pipeline_exclusion.py behind an IVF index that probes every list: the flat answers"""
    import torch
    from exclusion_ref import expected_excluding
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import path_tag
    from test_gpu_pipeline_exclusion import _CROWDED, _N, _pipeline, _store

    def pipeline(**knobs):
        pipe, cfg = _pipeline(gpu, tmp_path, index_type="IVF", **knobs)
        cfg.vector_db_nprobe = 64
        D = pipe.tpp.get_output_dim()
        db, q, paths, labels, query_paths = _store(D)
        pipe.vector_db.add_vectors(db, paths, labels, {"speaker_id": ["s"] * _N})
        assert pipe.vector_db.index.nlist == 64
        return pipe, cfg, db, torch.from_numpy(q).to(gpu), q, paths, labels, query_paths

    pipe, cfg, db, qd, q, paths, labels, query_paths = pipeline(ivf_exact_exclusion=True)
    K = cfg.top_k
    vec, lbl, rp, dist = pipe.retrieve_similar_vectors(qd, query_paths=query_paths, exclude_self=True, return_info=True, return_distances=True)
    names = {os.path.basename(p) for p in query_paths}
    assert all(x != "" and os.path.basename(x) not in names for row in rp for x in row)      # K real neighbours, none excluded
    tags = np.array([path_tag(p) for p in paths], np.int64)
    excl = np.unique([path_tag(p) for p in query_paths])
    ed, ei = expected_excluding(db, tags, excl, q, K, "L2")
    assert (ei >= 0).all()
    assert rp == [[paths[i] for i in row] for row in ei]
    np.testing.assert_array_equal(vec.cpu().numpy(), db[ei])
    np.testing.assert_array_equal(lbl.cpu().numpy(), np.asarray(labels, np.float32)[ei])
    np.testing.assert_allclose(dist.cpu().numpy(), ed, rtol=1e-6, atol=1e-5)
    assert pipe.vector_db.index.last_search_info()["scan"] in ("hi_lists", "f32_lists")
    assert len(pipe.retrieve_similar_vectors(qd, query_paths=query_paths)) == 2
    assert len(pipe.retrieve_similar_vectors(qd, query_paths=query_paths, return_info=True)) == 3
    assert len(pipe.retrieve_similar_vectors(qd, query_paths=query_paths, return_distances=True)) == 3
    # the flag off on the IVF store, and the flag on with a flat store (which ignores it): the padded result of the reference's loop
    od, oi = O.knn(db, q, K + 10, "L2")
    ov, ol, op, odist = O.retrieve_postprocess(od, oi, db, paths, labels, K, vec.shape[2], query_paths=query_paths, exclude_self=True)
    assert all(x == "" for j in range(_CROWDED) for x in op[j])
    pipe0, cfg0, *_ = pipeline()
    assert cfg0.ivf_exact_exclusion is False
    pipef, cfgf = _pipeline(gpu, tmp_path, index_type="L2", ivf_exact_exclusion=True)
    pipef.vector_db.add_vectors(db, paths, labels, {"speaker_id": ["s"] * _N})
    for pp in (pipe0, pipef):
        vec0, lbl0, rp0, dist0 = pp.retrieve_similar_vectors(qd, query_paths=query_paths, exclude_self=True, return_info=True, return_distances=True)
        assert rp0 == op
        np.testing.assert_array_equal(vec0.cpu().numpy(), ov)
        np.testing.assert_array_equal(lbl0.cpu().numpy(), ol)
        np.testing.assert_allclose(dist0.cpu().numpy(), odist, rtol=1e-5, atol=1e-5, equal_nan=True)
    with pytest.raises(ValueError, match="search_excluding"):          # the flat store's method of this kind has another name
        pipef.vector_db.search_probed_excluding(qd, 5, None)
    # exact_exclusion on an IVF store still raises, whatever the new flag says
    cfg.exact_exclusion = True
    with pytest.raises(ValueError, match="flat and single-handle only"):
        pipe.retrieve_similar_vectors(qd, query_paths=query_paths, exclude_self=True)
