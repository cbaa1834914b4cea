"""The IVF search with one exclusion set per query (radad_ivf_search_excl_pq, HipIVFFlatIndex.search_probed_excluding_per_query) against
the float64 model of tests/ivf_excl_pq_ref.py, through the four scan routes of tests/test_gpu_ivf_exclusion.py

  default   certified f16 list scan, k_ivf_scan_hi<per query>; rejected queries take k_ivf_exact<per query>
  f32       hi_scan=0: k_ivf_scan<KSEL, per query> behind its certificate
  rejected  hi_scan=2: k_ivf_exact<per query> answers every query
  noplane   dim 96: the fp32 list scan by itself

and with both values of RADAD_IVF_OPT_PQ_FILTER (1: the suspect pre-pass; 0: every row suspect, the per-(row, query) test decides
all of them).  ids must equal the model, distances agree to rtol 1e-6 / atol 1e-5, unfilled slots hold -1 / NaN.  What makes each case
the case it claims to be is asserted without a GPU by tests/test_ivf_excl_pq_model.py."""
import numpy as np
import pytest

from ivf_excl_pq_ref import KMAX, case, expected_pq
from oracle import synth
from test_gpu_ivf_adversarial import KS, NQS, _assert_route, _index
from test_gpu_ivf_exclusion import ROUTES, _build, _compare, _dev

pytestmark = pytest.mark.gpu
PQ_FILTER = (1, 0)


def _search(idx, gpu, q, k, tags, qtags, counts=None):
    D, I = idx.search_probed_excluding_per_query(_dev(gpu, q), k, None if tags is None else _dev(gpu, tags),
                                                 None if qtags is None else _dev(gpu, qtags), None if counts is None else _dev(gpu, counts))
    return D.cpu().numpy(), I.cpu().numpy()


def _check(idx, gpu, route, q, k, tags, qtags, counts, od, oi, what, failures):
    """one search under both settings of the pre-pass: the model's answer, the route, and the same bits either way"""
    got = []
    for pf in PQ_FILTER:
        idx.set_pq_filter(pf)
        D, I = _search(idx, gpu, q, k, tags, qtags, counts)
        info = idx.last_search_info()
        try:
            _compare(D, I, od, oi, k, None, (what, route, "pq_filter", pf))
            _assert_route(info, route, len(q), (what, route, pf))
        except (AssertionError, KeyError) as e:
            failures.append(f"{what} route {route} pq_filter {pf} nq {len(q)} k {k} {info}: {str(e)[:300]}")
        got.append((D, I))
    idx.set_pq_filter(1)
    if not (np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][0], got[1][0], equal_nan=True)):
        failures.append(f"{what} route {route} nq {len(q)} k {k}: RADAD_IVF_OPT_PQ_FILTER 0 and 1 differ")
    return got[0]


def _done(failures):
    assert not failures, f"{len(failures)} searches wrong:\n" + "\n".join(failures)


# ---- 1. twins in one task -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,dim", ROUTES)
def test_twins_in_one_task(gpu, route, dim):
    c = case("twins", dim)
    idx = _build(gpu, dim, c["cent"], c["db"], route, c["nprobe"])
    failures = []
    for nq in (2, 16, 17, 40):         # part of a task, one full task, one full task and a second, three tasks per probed list
        for k in (5, KMAX):
            D, I = _check(idx, gpu, route, c["q"][:nq], k, c["tags"], c["qtags"][:nq], c["counts"][:nq], c["od"][:nq], c["oi"][:nq],
                          "twins", failures)
    _done(failures)
    planted = set(c["planted_a"].tolist())
    assert set(I[1, :20].tolist()) == planted and not planted & set(I[0].tolist())
    rest = [i for i in I[1] if i not in planted]
    assert list(I[0, :len(rest)]) == rest and all(list(I[j]) == list(I[1]) for j in range(2, 40))


# ---- 2. crowded leave-one-out; 6. k across KS, nq across NQS -----------------------------------------------------------------------
@pytest.mark.parametrize("route,dim", ROUTES)
def test_crowded_leave_one_out(gpu, route, dim):
    c = case("loo", dim)
    idx = _build(gpu, dim, c["cent"], c["db"], route, c["nprobe"])
    failures = []
    for nq in NQS:
        sl = slice(3, 3 + nq) if nq < len(c["q"]) else slice(0, len(c["q"]))
        for k in KS:
            D, I = _check(idx, gpu, route, c["q"][sl], k, c["tags"], c["qtags"][sl], None, c["od"][sl], c["oi"][sl], "leave-one-out", failures)
    _done(failures)
    # (the last search: all 300 queries, k = 26) every planted query has its k neighbours, none of them its own near-copies; query 11
    # gets query 3's near-copies first
    for j, rows in zip(c["planted"], c["at"]):
        assert (I[j] >= 0).all() and not np.isin(I[j], rows).any()
    assert set(I[11, :20].tolist()) == set(c["at"][0].tolist())


# ---- 3. position coverage -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,dim", ROUTES)
def test_position_coverage(gpu, route, dim):
    c = case("positions", dim)
    idx = _build(gpu, dim, c["cent"], c["db"], route, c["nprobe"])
    np.testing.assert_array_equal(idx.assignments(), c["assign"])
    failures = []
    for k in (5, KMAX):
        _check(idx, gpu, route, c["q"], k, c["tags"], c["qtags"], c["counts"], c["od"], c["oi"], "run across 64 and 256", failures)
    # the whole home list excluded (the tag of a row is its list) beside a twin that excludes a list it does not probe
    for npb in (1, 3):
        idx.nprobe = npb
        od, oi = c[f"list{npb}"]
        D, I = _check(idx, gpu, route, c["q"][:2], 15, c["ltags"], c["list_qtags"], None, od, oi, f"home list excluded, nprobe {npb}", failures)
        if npb == 1:
            assert np.all(I[0] == -1) and np.all(np.isnan(D[0])) and np.all(I[1] >= 0)
        else:
            assert np.all(I >= 0)
    _done(failures)


@pytest.mark.parametrize("route,dim", ROUTES)
def test_split_lists(gpu, route, dim):
    """nq = 1 and 17 on lists of ~3750 rows: the f16 routes split every list over 8 workgroups (the reasoning of
    test_bit_indexing_in_split_lists), whose shares start on no multiple of 64"""
    c = case("long", dim)
    idx = _build(gpu, dim, c["cent"], c["db"], route, c["nprobe"])
    failures = []
    for sl in (slice(3, 4), slice(0, 17)):
        for k in (5, KMAX):
            _check(idx, gpu, route, c["q"][sl], k, c["tags"], c["qtags"][sl], None, c["od"][sl], c["oi"][sl], "split lists", failures)
    _done(failures)


# ---- 4. the set's shape -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,dim", ROUTES)
def test_the_shape_of_the_sets(gpu, route, dim):
    c = case("shapes", dim)
    idx = _build(gpu, dim, c["cent"], c["db"], route, c["nprobe"])
    failures = []
    for k in (15, KMAX):
        _check(idx, gpu, route, c["q"], k, c["tags"], c["qtags"], c["counts"], c["od"], c["oi"], "m 64, counts 0 / < 0 / > m / 9", failures)
        _check(idx, gpu, route, c["q"], k, c["tags"], c["qtags"], None, c["od_null"], c["oi_null"], "m 64, NULL counts", failures)
        _check(idx, gpu, route, c["q"], k, c["tags"], c["one"], None, c["od_one"], c["oi_one"], "m 1", failures)
        _check(idx, gpu, route, c["q"], k, c["tags"], c["one"][:, 0], None, c["od_one"], c["oi_one"], "m 1 as [nq]", failures)
    _done(failures)


# ---- 5. equivalences, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,dim", ROUTES)
def test_equivalences_bit_for_bit(gpu, route, dim):
    rng = np.random.default_rng(9997)
    c = case("loo", dim)
    q, tags = c["q"], c["tags"]
    idx = _build(gpu, dim, c["cent"], c["db"], route, c["nprobe"])
    same = lambda a, b: np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0], equal_nan=True)
    S = np.sort(1_000_000 + c["planted"]).astype(np.int64)
    rows = np.stack([rng.permutation(np.concatenate([S, S[:4]])) for _ in range(len(q))])      # any order, duplicates: m = 12
    none = -1 - np.arange(len(q) * 3, dtype=np.int64).reshape(len(q), 3)
    assert not np.isin(tags, none).any()
    for pf in PQ_FILTER:
        idx.set_pq_filter(pf)
        for nq, k in ((1, 5), (17, 15), (300, KMAX)):
            sl = slice(3, 3 + nq) if nq < 300 else slice(0, 300)
            # every query carries the same set: radad_ivf_search_excl with the set sorted
            Db, Ib = idx.search_probed_excluding(_dev(gpu, q[sl]), k, _dev(gpu, tags), _dev(gpu, S))
            assert same(_search(idx, gpu, q[sl], k, tags, rows[sl]), (Db.cpu().numpy(), Ib.cpu().numpy())), (route, pf, nq, k, "one set for all")
            _assert_route(idx.last_search_info(), route, len(q[sl]), (route, pf, nq, k))
            # nothing excluded: m == 0, counts all 0, tags no row carries -- radad_ivf_search on ids and filled distances
            D0, I0 = idx.search(q[sl], k)
            fin = I0 >= 0
            for qt, cn in ((None, None), (np.zeros((len(q[sl]), 0), np.int64), None), (rows[sl], np.zeros(len(q[sl]), np.int32)), (none[sl], None)):
                D, I = _search(idx, gpu, q[sl], k, tags, qt, cn)
                assert np.array_equal(I, I0) and np.array_equal(D[fin], D0[fin]) and np.all(np.isnan(D[~fin])), (route, pf, nq, k, "nothing excluded")
                _assert_route(idx.last_search_info(), route, len(q[sl]), (route, pf, nq, k))
        # a query answered in a batch of 300 and alone
        Dall, Iall = _search(idx, gpu, q, 15, tags, c["qtags"])
        for j in (3, 11, 12, 299):
            Dj, Ij = _search(idx, gpu, q[j:j + 1], 15, tags, c["qtags"][j:j + 1])
            assert same((Dj, Ij), (Dall[j:j + 1], Iall[j:j + 1])), (route, pf, j, "alone and in a batch of 300")
    idx.set_pq_filter(1)


# ---- 7. refusals, the empty index, Python, the pipeline ---------------------------------------------------------------------------
@pytest.mark.parametrize("route,dim", ROUTES)
def test_arguments_and_the_empty_index(gpu, route, dim):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    c = case("loo", dim)
    q, tags, qtags = c["q"][:4], c["tags"], c["qtags"][:4]
    idx = _index(gpu, dim, len(c["cent"]), route)
    with pytest.raises(ValueError, match="not trained"):
        _search(idx, gpu, q, 5, None, None)
    idx.set_centroids(c["cent"])
    idx.nprobe = 3
    D, I = _search(idx, gpu, q, 5, None, None)                             # a trained index without rows
    assert np.all(I == -1) and np.all(np.isnan(D))
    idx.add(c["db"])
    with pytest.raises(ValueError, match="26"):
        _search(idx, gpu, q, 27, tags, qtags)
    with pytest.raises(ValueError, match="at most 64"):
        _search(idx, gpu, q, 5, tags, np.zeros((4, 65), np.int64))
    with pytest.raises(ValueError, match="one tag per stored row"):
        _search(idx, gpu, q, 5, tags[:-1], qtags)
    with pytest.raises(ValueError, match="nq"):
        _search(idx, gpu, q, 5, tags, c["qtags"][:5])
    with pytest.raises(ValueError, match="search_probed_excluding_per_query"):      # the flat contract's method keeps refusing
        idx.search_excluding_per_query(_dev(gpu, q), 5, _dev(gpu, tags), _dev(gpu, qtags))
    qd, td, gd = _dev(gpu, q), _dev(gpu, tags), _dev(gpu, qtags)
    D = torch.empty((4, 27), device=gpu); I = torch.empty((4, 27), device=gpu, dtype=torch.int64)
    call = lambda k, rt, qt, m: idx._lib.radad_ivf_search_excl_pq(idx._h, qd.data_ptr(), 4, k, 3, rt, qt, m, None, D.data_ptr(), I.data_ptr(),
                                                                  _lib.stream_ptr(qd.device))
    assert call(27, td.data_ptr(), gd.data_ptr(), 1) == _lib.RADAD_EINVAL and b"26" in idx._lib.radad_last_error()
    assert call(5, td.data_ptr(), gd.data_ptr(), 65) == _lib.RADAD_EINVAL and call(5, td.data_ptr(), gd.data_ptr(), -1) == _lib.RADAD_EINVAL
    assert call(5, None, gd.data_ptr(), 1) == _lib.RADAD_EINVAL and call(5, td.data_ptr(), None, 1) == _lib.RADAD_EINVAL
    assert call(5, None, None, 0) == _lib.RADAD_OK
    assert idx._lib.radad_ivf_set_option(idx._h, _lib.IVF_OPT_PQ_FILTER, 2) == _lib.RADAD_EINVAL
    D, I = _search(idx, gpu, q, 5, tags, qtags)
    _compare(D, I, c["od"][:4], c["oi"][:4], 5, None, "after the refusals")
    info = idx.last_search_info()
    assert info["scan"] != "exact_flat" and idx.last_search_exact is False
    _assert_route(info, route, 4, route)


def test_pipeline_scope_query_on_an_ivf_store(gpu, tmp_path):
    """config.ivf_exact_exclusion + exclusion_scope 'query': a clip's neighbours do not change when a clip with another basename joins
    its batch; under scope 'batch' they do.  The store of tests/test_gpu_knn_excl_per_query.py behind an IVF index that probes every list"""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import path_tag
    import excl_per_query_ref as P
    from test_gpu_knn_excl_per_query import _two_clip_store
    from test_gpu_pipeline_exclusion import _pipeline
    pipe, cfg = _pipeline(gpu, tmp_path, index_type="IVF", ivf_exact_exclusion=True, exclusion_scope="query")
    cfg.vector_db_nprobe = 64
    D = pipe.tpp.get_output_dim()
    db, q, paths, labels, qpaths = _two_clip_store(D)
    pipe.vector_db.add_vectors(db, paths, labels, {"speaker_id": ["s"] * len(db)})
    assert pipe.vector_db.index.nlist == 64
    qd = torch.from_numpy(q).to(gpu)
    tags = np.array([path_tag(p) for p in paths], np.int64)
    own = np.array([[path_tag(p)] for p in qpaths], np.int64)
    _, ei = P.expected_pq(db, tags, own, None, q, cfg.top_k, "L2")             # (every list probed: the flat answer)
    assert ei[0, 0] == 20 and 10 not in ei[0]
    alone = pipe.retrieve_similar_vectors(qd[:1], query_paths=qpaths[:1], return_info=True, return_distances=True)
    both = pipe.retrieve_similar_vectors(qd, query_paths=qpaths, return_info=True, return_distances=True)
    assert alone[2][0] == both[2][0] == [paths[i] for i in ei[0]]
    assert both[2][1] == [paths[i] for i in ei[1]]
    assert torch.equal(alone[0][0], both[0][0]) and torch.equal(alone[1][0], both[1][0]) and torch.equal(alone[3][0], both[3][0])
    assert pipe.vector_db.index.last_search_info()["scan"] in ("hi_lists", "f32_lists")
    cfg.exclusion_scope = "batch"                                              # y's presence takes x's nearest neighbour away
    alone_b = pipe.retrieve_similar_vectors(qd[:1], query_paths=qpaths[:1], return_info=True)
    both_b = pipe.retrieve_similar_vectors(qd, query_paths=qpaths, return_info=True)
    assert alone_b[2][0] == alone[2][0] and both_b[2][0] != alone_b[2][0] and paths[20] not in both_b[2][0]
    cfg.exclusion_scope = "query"
    with pytest.raises(ValueError, match="query_paths"):
        pipe.retrieve_similar_vectors(qd)
    with pytest.raises(ValueError, match="one path per query"):
        pipe.retrieve_similar_vectors(qd, query_paths=qpaths[:1])
    # the database's method directly, and the flat store's method of this kind refused on an IVF store (and the other way round)
    Dd, Id = pipe.vector_db.search_probed_excluding_per_query(qd, cfg.top_k, own)
    np.testing.assert_array_equal(Id.cpu().numpy(), ei)
    with pytest.raises(ValueError, match="search_probed_excluding_per_query"):
        pipe.vector_db.search_excluding_per_query(qd, cfg.top_k, own)
    # what was refused stays refused: scope 'query' without either exact flag; exact_exclusion on an IVF store
    cfg.ivf_exact_exclusion = False
    with pytest.raises(ValueError, match="exact_exclusion"):
        pipe.retrieve_similar_vectors(qd, query_paths=qpaths)
    cfg.ivf_exact_exclusion = True
    cfg.exact_exclusion = True
    with pytest.raises(ValueError, match="flat and single-handle only"):
        pipe.retrieve_similar_vectors(qd, query_paths=qpaths)
    pipef, cfgf = _pipeline(gpu, tmp_path, index_type="L2", ivf_exact_exclusion=True, exclusion_scope="query")
    pipef.vector_db.add_vectors(db, paths, labels, {"speaker_id": ["s"] * len(db)})
    with pytest.raises(ValueError, match="exact_exclusion"):                   # a flat store ignores the IVF flag: the scope still needs exact_exclusion
        pipef.retrieve_similar_vectors(qd, query_paths=qpaths)
    with pytest.raises(ValueError, match="search_excluding_per_query"):
        pipef.vector_db.search_probed_excluding_per_query(qd, cfg.top_k, own)
