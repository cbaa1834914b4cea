"""Exclusion-aware flat search with one exclusion set PER QUERY (radad_knn_search_excl_pq / _pq_begin,
HipFlatIndex.search_excluding_per_query): row r is admissible for query j iff its tag is not among the first cnt_j of the query's own
<= 64 tags.  The batch-wide form (tests/test_gpu_knn_exclusion.py) excludes the union of the batch, so what a clip retrieves depends
on its batch; here it is a function of the query alone.

Reference (tests/excl_per_query_ref.py, checked on the CPU by tests/test_excl_per_query_model.py): per query the float64 oracle over
the rows AS STORED that the query admits.  The number of queries that take the exact pass is derived from the oracle's top-k_fetch
over the whole store and asserted with equality.  Tolerances: those of tests/test_gpu_knn_exclusion.py (ids equal; 1e-4 absolute on
unit-norm data, rtol / atol 1e-6 on raw L2; K64.astype(float32) == D on filled slots).

The new way to go wrong: the <= 8 queries of one exact-pass group have DIFFERENT admissible sets (the `mutual` store: eight identical
query vectors per group, eight different sets)."""
import numpy as np
import pytest

import excl_per_query_ref as P
from exclusion_ref import crowded
from sharded_excl_ref import bases_of, own_flags

pytestmark = pytest.mark.gpu


def _mk(metric, dim, f16=False, id_base=0):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    return HipFlatIndex(dim, m, 0, id_base, store_f16=f16)


def _stored(idx, n, gpu):
    import torch
    ids = torch.arange(idx.id_base, idx.id_base + n, device=gpu)
    return idx.reconstruct_batch(ids).cpu().numpy()


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _check(D, I, ed, ei, metric, K64=None):
    D, I = D.cpu().numpy(), I.cpu().numpy()
    np.testing.assert_array_equal(I, ei)
    f = ei >= 0
    if metric == "COSINE":
        np.testing.assert_allclose(D[f], ed[f], rtol=0, atol=1e-4)
    else:
        np.testing.assert_allclose(D[f], ed[f], rtol=1e-6, atol=1e-6)
    assert np.all(np.isnan(D[~f]))
    if K64 is not None:
        K64 = K64.cpu().numpy()
        assert np.all(np.isnan(K64[~f]))
        np.testing.assert_array_equal(K64[f].astype(np.float32), D[f])          # out_dist is the key, rounded once


def _bits_equal(a, b):
    import torch
    w = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.view(w), b.view(w))              # (NaN padding included)


class _Case:
    """a store on the device, its rows as stored, row tags and the queries' own tags / counts; the reference is computed once per
    (k, metric) for all queries and sliced: a query's answer does not depend on the batch"""

    def __init__(self, gpu, metric, store, f16=False, id_base=0):
        db, q, tags, qtags, qcnt = store[:5]
        self.metric, self.q, self.tags, self.qtags, self.qcnt, self.gpu = metric, q, np.asarray(tags, np.int64), qtags, qcnt, gpu
        self.info = store[5] if len(store) > 5 else None
        self.idx = _mk(metric, db.shape[1], f16, id_base)
        self.idx.add(db)
        self.stored = _stored(self.idx, len(db), gpu)
        self.tags_t, self.qtags_t = _dev(self.tags, gpu), _dev(qtags, gpu)
        self.qcnt_t = None if qcnt is None else _dev(np.asarray(qcnt, np.int32), gpu)
        self._ref = {}

    def want(self, k, q_ref=None):
        if q_ref is not None:
            return P.expected_pq(self.stored, self.tags, self.qtags[:len(q_ref)], None if self.qcnt is None else self.qcnt[:len(q_ref)],
                                 q_ref, k, self.metric, self.idx.id_base)
        if k not in self._ref:
            self._ref[k] = P.expected_pq(self.stored, self.tags, self.qtags, self.qcnt, self.q, k, self.metric, self.idx.id_base)
        return self._ref[k]

    def listed(self, k, k_fetch, q_ref=None):
        q = self.q if q_ref is None else q_ref
        n = len(q)
        return P.expected_exact_pq(self.stored, self.tags, self.qtags[:n], None if self.qcnt is None else self.qcnt[:n], q, k, k_fetch,
                                   self.metric)

    def run(self, k, k_fetch, nq=None, q=None, q_ref=None, return_f64=False):
        """search the first nq queries, compare with the reference, assert the derived exact-pass count; -> (count, ids)"""
        nq = len(self.q) if nq is None else nq
        qt = _dev(self.q[:nq], self.gpu) if q is None else q
        cnt = None if self.qcnt_t is None else self.qcnt_t[:nq]
        out = self.idx.search_excluding_per_query(qt, k, self.tags_t, self.qtags_t[:nq], cnt, k_fetch=k_fetch, return_f64=return_f64)
        ed, ei = self.want(k, q_ref)
        want = int(self.listed(k, k_fetch, q_ref)[:nq].sum())
        info = self.idx.last_excl()
        print(f"exact pass: {info['exact']} of {info['queries']} queries (derived {want}), scan {self.idx.last_launch()['scan_kind']}")
        _check(out[0], out[1], ed[:nq], ei[:nq], self.metric, out[2] if return_f64 else None)
        assert info == {"queries": nq, "exact": want}, (info, want)
        return want, out[1].cpu().numpy()


# ---- 1. leave-one-out: a query excludes its own file -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_leave_one_out(gpu, metric):
    c = _Case(gpu, metric, P.per_file(20000, 64, 40, 3, 13, 9301))
    # no tag is carried by more than c = 3 rows, m = 1: k_fetch = k + m c proves every query in the fast pass
    n_exact, I = c.run(5, 8, return_f64=True)
    assert n_exact == 0
    for j in c.info:
        assert not np.isin(c.tags[I[j]], c.qtags[j]).any()
    n_exact, _ = c.run(5, 7, return_f64=True)                        # one short: exactly the 13 owning queries are listed
    assert n_exact == 13


# ---- 2. same vector, different sets -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mutual_cases(gpu):
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = _Case(gpu, metric, P.mutual(20000, 64, 5, 9402))
        return cache[metric]
    yield get
    cache.clear()


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_same_vector_different_sets(gpu, mutual_cases, metric):
    import torch
    c = mutual_cases(metric)
    n_exact, I = c.run(5, 10, return_f64=True)
    assert n_exact > 8 and n_exact % 8 != 0                          # full groups and a tail group of the exact pass
    _, ei = c.want(5)
    for g in range(5):
        got = len({tuple(r) for r in I[8 * g:8 * g + 8]})
        assert got == len({tuple(r) for r in ei[8 * g:8 * g + 8]}) >= 2, (g, got)
    # the contrast: the batch-wide form with the UNION of all tags gives the 8 identical queries of a group one identical list
    union = torch.unique(c.qtags_t.reshape(-1))
    _, Iu = c.idx.search_excluding(_dev(c.q, gpu), 5, c.tags_t, union, k_fetch=10)
    Iu = Iu.cpu().numpy()
    for g in range(5):
        assert len({tuple(r) for r in Iu[8 * g:8 * g + 8]}) == 1


# ---- 7. batch independence --------------------------------------------------------------------------------------------------------------
def test_batch_independence(gpu, mutual_cases):
    c = mutual_cases("L2")
    qt = _dev(c.q, gpu)
    _, I = c.idx.search_excluding_per_query(qt, 5, c.tags_t, c.qtags_t, c.qcnt_t, k_fetch=10)
    _, ei = c.want(5)
    for j in range(40):
        _, Ij = c.idx.search_excluding_per_query(qt[j:j + 1], 5, c.tags_t, c.qtags_t[j:j + 1], c.qcnt_t[j:j + 1], k_fetch=10)
        assert Ij.cpu().numpy().tolist() == I[j:j + 1].cpu().numpy().tolist() == ei[j:j + 1].tolist(), j


# ---- 3. every fast-pass route and store ---------------------------------------------------------------------------------------------------
_ROUTES = {"dense": (4096, 64, "L2", False), "hi_plane": (20000, 64, "COSINE", False), "fp32": (20000, 36, "L2", False),
           "f16_store": (20000, 64, "L2", True)}


@pytest.fixture(scope="module")
def route_cases(gpu):
    cache = {}

    def get(name):
        if name not in cache:
            n, dim, metric, f16 = _ROUTES[name]
            cache[name] = _Case(gpu, metric, P.per_file(n, dim, 40, 3, 13, 9310 + len(cache)), f16=f16)
        return cache[name]
    yield get
    cache.clear()


@pytest.mark.parametrize("k_fetch", [7, 200])
@pytest.mark.parametrize("nq", [1, 16, 17, 40])
@pytest.mark.parametrize("route", ["dense", "hi_plane", "fp32", "f16_store"])
def test_fast_pass_routes(gpu, route_cases, route, nq, k_fetch):
    c = route_cases(route)
    n_exact, _ = c.run(5, k_fetch, nq=nq)
    kind = c.idx.last_launch()["scan_kind"]
    if k_fetch == 200:
        assert n_exact == 0
        assert kind == ("f32_dense" if route == "dense" else "f32_tile"), kind      # above 128: no f16 scan
    else:
        assert n_exact == int(np.sum(c.info < nq))                    # the owning queries among the first nq
    if route == "dense":
        assert kind == "f32_dense", kind
    if route == "hi_plane" and k_fetch == 7:
        assert kind == ("hi_tile" if nq > 16 else "hi_smallq"), kind
    if route == "fp32":
        assert kind == "f32_tile", kind


def test_bf16_queries(gpu, route_cases):
    import torch
    c = route_cases("hi_plane")
    qb = torch.from_numpy(c.q).to(gpu).bfloat16()
    n_exact, _ = c.run(5, 7, q=qb, q_ref=qb.float().cpu().numpy())
    assert n_exact == 13


# ---- 4. equal sets for every query == the batch-wide form, bit for bit --------------------------------------------------------------------
def test_equal_sets_are_the_batch_form(gpu):
    db, q, tags, excl, which = crowded(20000, 64, 40, 4, 12, 9401, extra_excl=16)
    assert len(excl) == 64                                            # m = 64: a full-wave ballot
    idx = _mk("L2", 64)
    idx.add(db)
    qt, tags_t, excl_t = _dev(q, gpu), _dev(tags, gpu), _dev(excl, gpu)
    qtags_t = _dev(np.tile(excl[::-1], (40, 1)), gpu)                 # any order
    D0, I0, K0 = idx.search_excluding(qt, 5, tags_t, excl_t, k_fetch=15, return_f64=True)
    info0 = idx.last_excl()
    D1, I1, K1 = idx.search_excluding_per_query(qt, 5, tags_t, qtags_t, None, k_fetch=15, return_f64=True)
    info1 = idx.last_excl()
    print(f"batch form {info0}, per-query form {info1}")
    assert info0 == info1 and info1["exact"] > 0
    assert _bits_equal(I1, I0) and _bits_equal(D1, D0) and _bits_equal(K1, K0)


# ---- 5. nothing excluded; counts are clamped ---------------------------------------------------------------------------------------------
def test_nothing_excluded(gpu, mutual_cases):
    import torch
    c = mutual_cases("COSINE")
    qt = _dev(c.q, gpu)
    D0, I0 = c.idx.search_device(qt, 5)
    for qtags, cnt in ((torch.empty((40, 0), dtype=torch.int64, device=gpu), None),                      # m = 0
                       (c.qtags_t[:, :3].contiguous(), torch.zeros(40, dtype=torch.int32, device=gpu)),  # m = 3, every count 0
                       (None, None)):
        D, I, K64 = c.idx.search_excluding_per_query(qt, 5, c.tags_t, qtags, cnt, k_fetch=10, return_f64=True)
        assert c.idx.last_excl() == {"queries": 40, "exact": 0}
        assert torch.equal(I, I0) and torch.equal(D, D0) and torch.equal(K64.float(), D0)


def test_counts_are_clamped_on_the_device(gpu, mutual_cases):
    c = mutual_cases("L2")
    cnt = np.where(np.arange(40) % 2 == 0, 100, -5).astype(np.int32)  # above m behaves as m, negative as 0
    D, I = c.idx.search_excluding_per_query(_dev(c.q, gpu), 5, c.tags_t, c.qtags_t, _dev(cnt, gpu), k_fetch=10)
    ed, ei = P.expected_pq(c.stored, c.tags, c.qtags, np.where(np.arange(40) % 2 == 0, c.qtags.shape[1], 0), c.q, 5, "L2")
    want = int(P.expected_exact_pq(c.stored, c.tags, c.qtags, cnt, c.q, 5, 10, "L2").sum())
    assert c.idx.last_excl() == {"queries": 40, "exact": want}
    _check(D, I, ed, ei, "L2")


# ---- 6. groups, tails, large k ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nearest_case(gpu):
    yield _Case(gpu, "L2", P.nearest(3000, 64, 19, 9501))


@pytest.mark.parametrize("k,k_fetch", [(5, 15), (130, 140), (1024, 1024)])
def test_groups_tails_large_k(gpu, nearest_case, k, k_fetch):
    """every query excludes its own 20 nearest rows (m = 20): all 19 are listed -- two full groups of eight and a tail of three at
    k <= 130, groups of one at k = 1024"""
    n_exact, I = nearest_case.run(k, k_fetch, return_f64=True)
    assert n_exact == 19
    for j in range(19):
        assert not np.isin(I[j], nearest_case.info[j]).any()


# ---- 8. shards on one GPU -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store,metric", [("mutual", "L2"), ("mutual", "COSINE"), ("per_file", "L2")])
def test_shards_on_one_gpu(gpu, store, metric):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import hip_merge
    sizes, k, k_fetch = [2500, 2500, 1000], 5, 6
    db, q, tags, qtags, qcnt = (P.mutual(6000, 64, 5, 9402) if store == "mutual" else P.per_file(6000, 64, 40, 3, 13, 9301))[:5]
    b = bases_of(sizes)
    whole = _Case(gpu, metric, (db, q, tags, qtags, qcnt))
    shards = [_Case(gpu, metric, (db[b[g]:b[g + 1]], q, tags[b[g]:b[g + 1]], qtags, qcnt), id_base=int(b[g])) for g in range(3)]
    qt = _dev(q, gpu)
    _, I_whole = whole.run(k, k_fetch)
    ed, ei = whole.want(k)
    begun = [s.idx.search_excluding_per_query_begin(qt, k, s.tags_t, s.qtags_t, s.qcnt_t, k_fetch) for s in shards]
    for s in shards:
        assert s.idx.last_excl() == {"queries": len(q), "exact": 0}
    K, I, FK, FI = (torch.stack([x[c] for x in begun]) for c in range(4))
    for g, s in enumerate(shards):                                    # the shard halves are the model's
        mk, mi, mfk, mfi = P.shard_begin_pq(s.stored, s.tags, qtags, qcnt, q, k, k_fetch, metric, int(b[g]))
        np.testing.assert_array_equal(I[g].cpu().numpy(), mi)
        np.testing.assert_array_equal(FI[g].cpu().numpy(), mfi)
    m = shards[0].idx.metric
    D, Im, K64, U = HipFlatIndex.excl_merge_certify(m, K, I, FK, FI)
    _, _, want_u = P.sharded_search_excluding_pq(whole.stored, tags, qtags, qcnt, q, k, k_fetch, metric, sizes)
    np.testing.assert_array_equal(U.cpu().numpy(), want_u)
    assert want_u.any()
    done = [s.idx.search_excluding_finish(U, return_f64=True) for s in shards]
    K2, I2 = torch.stack([x[2] for x in done]), torch.stack([x[1] for x in done])
    D, Im = hip_merge(m, K2, I2, k)
    D = D.masked_fill(Im < 0, float("nan"))
    _check(D, Im, ed, ei, metric)
    np.testing.assert_array_equal(Im.cpu().numpy(), I_whole)
    # _pq_begin + _finish with the shard's OWN flags is the single call on that shard, bit for bit
    for g, s in enumerate(shards):
        D1, I1, K1 = s.idx.search_excluding_per_query(qt, k, s.tags_t, s.qtags_t, s.qcnt_t, k_fetch=k_fetch, return_f64=True)
        info1 = s.idx.last_excl()
        Kb, Ib, FKb, FIb = s.idx.search_excluding_per_query_begin(qt, k, s.tags_t, s.qtags_t, s.qcnt_t, k_fetch)
        own = own_flags(Ib.cpu().numpy(), FIb.cpu().numpy())
        D2, I2_, K2_ = s.idx.search_excluding_finish(_dev(own.astype(np.int32), gpu), return_f64=True)
        assert s.idx.last_excl() == info1 == {"queries": len(q), "exact": int(own.sum())}
        assert _bits_equal(I2_, I1) and _bits_equal(D2, D1) and _bits_equal(K2_, K1)
    # search_abort after _pq_begin frees the handle
    s = shards[0]
    s.idx.search_excluding_per_query_begin(qt, k, s.tags_t, s.qtags_t, s.qcnt_t, k_fetch)
    with pytest.raises(ValueError):
        s.idx.search_device(qt, k)
    s.idx.search_abort()
    with pytest.raises(ValueError):
        s.idx.search_excluding_finish(None)
    s.idx.search_device(qt, k)


# ---- 9. errors --------------------------------------------------------------------------------------------------------------------------
def test_errors(gpu, mutual_cases):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    c = mutual_cases("L2")
    lib = _lib.load()
    qt = _dev(c.q[:20], gpu)
    D0, I0 = c.idx.search_device(qt, 5)
    D = torch.empty((20, 5), device=gpu)
    I = torch.empty((20, 5), device=gpu, dtype=torch.int64)
    big = torch.zeros((20, 65), dtype=torch.int64, device=gpu)

    def call(tags, qtags, m, k=5, k_fetch=10, h=None):
        return lib.radad_knn_search_excl_pq(h or c.idx._h, qt.data_ptr(), _lib.Q_F32, 20, k, k_fetch, tags, qtags, m, None, D.data_ptr(),
                                            I.data_ptr(), None, _lib.stream_ptr(gpu))
    assert call(c.tags_t.data_ptr(), big.data_ptr(), 65) == _lib.RADAD_EINVAL                 # m above the limit ...
    assert "64" in lib.radad_last_error().decode()                                            # ... and the message names it
    assert call(c.tags_t.data_ptr(), None, 2) == _lib.RADAD_EINVAL                            # m = 2 without the query tags
    assert call(None, c.qtags_t.data_ptr(), 2) == _lib.RADAD_EINVAL                           # ... or without the row tags
    assert call(c.tags_t.data_ptr(), c.qtags_t.data_ptr(), -1) == _lib.RADAD_EINVAL
    assert call(c.tags_t.data_ptr(), c.qtags_t.data_ptr(), 8, k_fetch=4) == _lib.RADAD_EINVAL
    empty = _mk("L2", 64)
    assert call(c.tags_t.data_ptr(), c.qtags_t.data_ptr(), 8, h=empty._h) == _lib.RADAD_ESTATE
    FK = torch.empty((20,), device=gpu, dtype=torch.float64)
    FI = torch.empty((20,), device=gpu, dtype=torch.int64)
    K64 = torch.empty((20, 5), device=gpu, dtype=torch.float64)
    assert lib.radad_knn_search_excl_pq_begin(empty._h, qt.data_ptr(), _lib.Q_F32, 20, 5, 10, c.tags_t.data_ptr(), c.qtags_t.data_ptr(), 8,
                                              None, K64.data_ptr(), I.data_ptr(), FK.data_ptr(), FI.data_ptr(),
                                              _lib.stream_ptr(gpu)) == _lib.RADAD_ESTATE
    assert lib.radad_knn_search_excl_pq_begin(c.idx._h, qt.data_ptr(), _lib.Q_F32, 20, 5, 10, c.tags_t.data_ptr(), big.data_ptr(), 65,
                                              None, K64.data_ptr(), I.data_ptr(), FK.data_ptr(), FI.data_ptr(),
                                              _lib.stream_ptr(gpu)) == _lib.RADAD_EINVAL
    # the Python surface: too many tags, tags on the CPU, wrong shapes
    with pytest.raises(ValueError, match="64"):
        c.idx.search_excluding_per_query(qt, 5, c.tags_t, big)
    with pytest.raises(ValueError, match="CUDA"):
        c.idx.search_excluding_per_query(qt, 5, c.tags_t, c.qtags_t[:20].cpu())
    with pytest.raises(ValueError, match="CUDA"):
        c.idx.search_excluding_per_query(qt, 5, c.tags_t.cpu(), c.qtags_t[:20])
    with pytest.raises(ValueError):
        c.idx.search_excluding_per_query(qt, 5, c.tags_t, c.qtags_t[:19])
    with pytest.raises(ValueError):
        c.idx.search_excluding_per_query(qt, 5, c.tags_t[:100], c.qtags_t[:20])
    with pytest.raises(ValueError):
        c.idx.search_excluding_per_query(qt, 5, c.tags_t, c.qtags_t[:20], c.qcnt_t[:3])
    # any search while one is begun is refused, of either kind
    c.idx.search_excluding_per_query_begin(qt, 5, c.tags_t, c.qtags_t[:20], c.qcnt_t[:20], 10)
    for refused in (lambda: c.idx.search_excluding_per_query(qt, 5, c.tags_t, c.qtags_t[:20]),
                    lambda: c.idx.search_excluding_per_query_begin(qt, 5, c.tags_t, c.qtags_t[:20]),
                    lambda: c.idx.search_excluding(qt, 5, c.tags_t, None),
                    lambda: c.idx.search_device(qt, 5)):
        with pytest.raises(ValueError):
            refused()
    assert call(c.tags_t.data_ptr(), c.qtags_t.data_ptr(), 8) == _lib.RADAD_EINVAL
    c.idx.search_abort()
    c.idx.search_begin(qt, 5)
    with pytest.raises(ValueError):
        c.idx.search_excluding_per_query(qt, 5, c.tags_t, c.qtags_t[:20])
    c.idx.search_abort()
    D1, I1 = c.idx.search_device(qt, 5)                               # after the refused calls a plain search still works
    assert torch.equal(I1, I0) and torch.equal(D1, D0)
    c.run(5, 10, nq=20)


# ---- 10. the pipeline: config.exclusion_scope ---------------------------------------------------------------------------------------------
def _pipeline(gpu, tmp_path, **knobs):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, feature_dim=32, tpp_levels=[1, 2], top_k=5, vector_db_index_type="L2",
               vector_db_path=str(tmp_path / ("vdb_" + "_".join(knobs))), **knobs)

    class NoExtractor:
        feature_dim = 32

        def extract_features(self, segments):
            raise AssertionError("not used")
    return R.HotPathPipeline(cfg, feature_extractor=NoExtractor()), cfg


def _two_clip_store(D):
    """clip x's nearest admissible neighbour is clip y's own file row: row 20 is stored under y's basename and lies near x"""
    from oracle import synth
    rng = np.random.default_rng(9911)
    n = 4096
    db = synth.rows(0, n, D, 9901)
    q = synth.rows(0, 2, D, 9902)
    paths = [f"/train/f{i}.wav" for i in range(n)]
    db[10] = q[0] + 1e-3 * rng.standard_normal(D)
    paths[10] = "/train/clipx.wav"
    db[20] = q[0] + 0.1 * rng.standard_normal(D)
    paths[20] = "/train/clipy.wav"
    return db, q, paths, [float(i % 2) for i in range(n)], ["/eval/clipx.wav", "/eval/clipy.wav"]


def test_pipeline_exclusion_scope(gpu, tmp_path):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.vector_database import path_tag
    pipe, cfg = _pipeline(gpu, tmp_path, exact_exclusion=True, exclusion_scope="query")
    D = pipe.tpp.get_output_dim()
    db, q, paths, labels, qpaths = _two_clip_store(D)
    pipe.vector_db.add_vectors(db, paths, labels, {"speaker_id": ["s"] * len(db)})
    qd = torch.from_numpy(q).to(gpu)
    tags = np.array([path_tag(p) for p in paths], np.int64)
    own = np.array([[path_tag(p)] for p in qpaths], np.int64)
    _, ei = P.expected_pq(db, tags, own, None, q, cfg.top_k, "L2")
    assert ei[0, 0] == 20 and 10 not in ei[0]
    alone = pipe.retrieve_similar_vectors(qd[:1], query_paths=qpaths[:1], return_info=True, return_distances=True)
    both = pipe.retrieve_similar_vectors(qd, query_paths=qpaths, return_info=True, return_distances=True)
    assert alone[2][0] == both[2][0] == [paths[i] for i in ei[0]]     # x: the same neighbours alone and beside y
    assert both[2][1] == [paths[i] for i in ei[1]]
    assert torch.equal(alone[0][0], both[0][0]) and torch.equal(alone[1][0], both[1][0])
    cfg.exclusion_scope = "batch"                                     # the default scope: y's presence takes x's nearest neighbour away
    alone_b = pipe.retrieve_similar_vectors(qd[:1], query_paths=qpaths[:1], return_info=True)
    both_b = pipe.retrieve_similar_vectors(qd, query_paths=qpaths, return_info=True)
    assert alone_b[2][0] == alone[2][0] and both_b[2][0] != alone_b[2][0] and paths[20] not in both_b[2][0]
    cfg.exclusion_scope = "query"
    with pytest.raises(ValueError, match="query_paths"):
        pipe.retrieve_similar_vectors(qd)
    cfg.exact_exclusion = False
    with pytest.raises(ValueError, match="exact_exclusion"):
        pipe.retrieve_similar_vectors(qd, query_paths=qpaths)
    vec, lbl = pipe.retrieve_similar_vectors(qd, query_paths=qpaths, exclude_self=False)    # the scope needs exclude_self
    assert vec.shape == (2, cfg.top_k, D)
    cfg.exclusion_scope = "speaker"
    with pytest.raises(ValueError, match="exclusion_scope"):
        pipe.retrieve_similar_vectors(qd, query_paths=qpaths)
