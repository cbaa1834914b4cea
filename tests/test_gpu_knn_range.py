"""Certified range search (radad_knn_range_search / HipFlatIndex.range_search): every stored row within a radius of each query,
exactly -- the exact count, the best max_per_query rows in (float64 key, lower id) order, -1 / NaN / NaN in the other slots.

Expected results: tests/range_ref.expected_range, float64 numpy over the rows AS STORED (under cosine: their inner product with the
device's radad_rownorm of the query).  Counts and ids are compared exactly; keys within 1e-4 absolute on unit-norm data under
cosine, 1e-6 relative and absolute on raw L2 / IP (the siblings' tolerances); float32(key) == dist bit for bit.  The stores are
tests/range_ref.case's: tests/test_range_model.py asserts on the CPU that none has a row within 1e-9 of its radius (the integer stores
apart, whose keys are exact) and that no query of the tile route can overflow its 4096-entry buffer while the scan's eps stays below
range_ref.EPS_MODEL.  Every tile-route case measures that eps -- the threshold minus the floor the scan ran with
(radad_knn_last_emitted) -- and fails, naming the constant, when it is larger.

Measured on an MI355X (largest threshold - floor over the batch): see profiles/README.md, "Range search"."""
import logging
import os

import numpy as np
import pytest

import range_ref as R

pytestmark = pytest.mark.gpu


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _rownorm(gpu, q):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    qt = _dev(np.asarray(q, np.float32), gpu)
    out = torch.empty_like(qt)
    _lib.check(_lib.load().radad_rownorm(qt.data_ptr(), out.data_ptr(), qt.shape[0], qt.shape[1], gpu.index or 0, _lib.stream_ptr(gpu)))
    return out.cpu().numpy()


def _mk(metric, dim, kind="uncentred", id_base=0, **kw):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipFlatIndex, _lib
    m = {"L2": _lib.METRIC_L2, "IP": _lib.METRIC_IP, "COSINE": _lib.METRIC_COSINE}[metric]
    if kind == "f16":
        return HipFlatIndex(dim, m, 0, id_base, store_f16=True, **kw)
    return HipFlatIndex(dim, m, 0, id_base, centre=1 if kind == "centred" else 0, **kw)


class _Store:
    """a handle holding a designed case's rows, and the rows as it stores them"""

    def __init__(self, gpu, c, id_base=0, **kw):
        self.gpu, self.metric, self.kind, self.id_base, self.c = gpu, c["metric"], c["kind"], id_base, c
        self.idx = _mk(self.metric, c["db"].shape[1], self.kind, id_base, **kw)
        self.idx.add_device(_dev(np.asarray(c["db"], np.float32), gpu))
        self.refresh()

    def refresh(self):
        import torch
        n, b = self.idx.ntotal, self.id_base
        self.stored = np.concatenate([self.idx.reconstruct_batch(torch.arange(b + r0, b + min(n, r0 + 65536), device=self.gpu)).cpu().numpy()
                                      for r0 in range(0, n, 65536)])

    def run(self, q, radius, M, bf16=False):
        import torch
        qt = _dev(np.asarray(q, np.float32), self.gpu)
        if bf16:
            qt = qt.to(torch.bfloat16)
        counts, D, I, K64 = self.idx.range_search_device(qt, radius, M, return_f64=True)
        return counts, D, I, K64, self.idx.last_range()

    def reference(self, q, radius, M):
        """range_ref.expected_range over the rows as stored; the float64 keys of a batch are computed once per store"""
        metric = "IP" if self.metric == "COSINE" else self.metric
        tag = (len(self.stored), np.asarray(q, np.float32).tobytes())
        if getattr(self, "_keys_of", None) != tag:
            self._keys = R.keys(self.stored, _rownorm(self.gpu, q) if self.metric == "COSINE" else q, metric)
            self._keys_of = tag
        return R.expected_range(self.stored, q, radius, metric, M, self.id_base, key=self._keys)


def _check(out, ref, metric, M):
    counts, D, I, K64 = (t.cpu().numpy() for t in out[:4])
    ec, ei, ek, boundary = ref
    assert not boundary.any() or metric in ("IP", "L2"), "boundary rows in a store that should have none"
    np.testing.assert_array_equal(counts, ec)
    np.testing.assert_array_equal(I, ei)
    f = ei >= 0
    np.testing.assert_array_equal(f.sum(axis=1), np.minimum(ec, M))
    if metric == "COSINE":
        np.testing.assert_allclose(K64[f], ek[f], rtol=0, atol=1e-4)
    else:
        np.testing.assert_allclose(K64[f], ek[f], rtol=1e-6, atol=1e-6)
    assert np.all(np.isnan(D[~f])) and np.all(np.isnan(K64[~f]))                    # padding: -1 / NaN / NaN
    np.testing.assert_array_equal(K64[f].astype(np.float32), D[f])                  # out_dist is the key, rounded once


def _expect_tile(s, info, nq, radius, n_exact=0):
    """the tile route ran, `n_exact` queries went to the exact pass, and the scan's eps is within the model's"""
    assert info["route"] == "tile" and info["queries"] == nq, info
    if n_exact is not None:
        assert info["exact"] == n_exact, info
    emitted, floors = s.idx.last_emitted(nq)
    launch = s.idx.last_launch()
    assert launch["scan_launches"] == 1 and launch["scan_phases"] == 1, launch
    if np.isfinite(radius):
        T = -radius if s.metric == "L2" else radius
        eps = np.float64(T) - floors.astype(np.float64)
        print(f"{s.c['name']} {s.metric} nq {nq}: measured eps (threshold - floor) max {eps.max():.3e} min {eps.min():.3e}; "
              f"emitted max {emitted.max()}; {info}")
        assert (eps > 0).all()
        assert eps.max() <= R.EPS_MODEL[s.metric], \
            f"the scan's eps {eps.max():.3e} exceeds range_ref.EPS_MODEL[{s.metric!r}] = {R.EPS_MODEL[s.metric]}: widen the constant, re-check the CPU caps"
    return emitted


@pytest.fixture(scope="module")
def stores(gpu):
    """one handle per designed case, built once"""
    cache = {}

    def get(name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in cache:
            cache[key] = _Store(gpu, R.case(name), **kw)
        return cache[key]
    yield get
    cache.clear()


# ---- 1, 2, 3, 4: graded neighbours on the tile route -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["graded_cosine", "graded_l2", "graded_ip", "centred", "graded_f16", "graded_bf16"])
def test_1_graded_neighbours(gpu, stores, name):
    s = stores(name)
    c = s.c
    if name == "centred":
        s.idx.search_device(_dev(c["q"], gpu), 1)                                    # (builds the plane)
        assert s.idx.plane_info()["centred"], s.idx.plane_info()
    for nq in (17, 300):
        q = c["q"][:nq]
        ref = s.reference(q, c["radius"], c["M"])
        out = s.run(q, c["radius"], c["M"], bf16=name == "graded_bf16")
        _check(out, ref, s.metric, c["M"])
        _expect_tile(s, out[4], nq, c["radius"])
        np.testing.assert_array_equal(ref[0], [R.COUNTS[j % 4] for j in range(nq)])   # the planted rows, nothing else
        for j in (1, 2, 3):
            np.testing.assert_array_equal(np.sort(out[2][j, :ref[0][j]].cpu().numpy()), np.sort(c["info"]["planted_in"][j]))


# ---- 5: strictness on exact keys -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["integer_ip", "integer_l2"])
def test_5_rows_that_hit_the_radius_are_out(gpu, stores, name):
    s = stores(name)
    c = s.c
    np.testing.assert_array_equal(s.stored, c["db"])
    for nq in (17, 300):
        q = c["q"][:nq]
        for radius in (c["radius"], c["radius"] - 1, c["radius"] + 1):
            ref = s.reference(q, radius, c["M"])
            out = s.run(q, radius, c["M"])
            _check(out, ref, s.metric, c["M"])
            _expect_tile(s, out[4], nq, radius)
            K64 = out[3].cpu().numpy()
            filled = ref[1] >= 0
            assert (K64[filled] < radius).all() if s.metric == "L2" else (K64[filled] > radius).all()      # strictly
            if radius == c["radius"]:
                assert ref[3].any(axis=1).sum() >= nq // 2                           # rows that hit it exactly exist, and are out
                np.testing.assert_array_equal(K64[filled], np.round(K64[filled]))    # integers
    rows = np.concatenate([[c["info"]["best"]], c["info"]["copies"]])
    np.testing.assert_array_equal(out[2][0, :len(rows)].cpu().numpy(), rows)         # duplicates of one row: id order


# ---- 6: truncation on the tile route -----------------------------------------------------------------------------------------------------
def test_6_a_list_cut_to_max_per_query_keeps_the_exact_count(gpu, stores):
    s = stores("truncation")
    c = s.c
    assert c["M"] == 16
    ref = s.reference(c["q"], c["radius"], c["M"])
    out = s.run(c["q"], c["radius"], c["M"])
    _check(out, ref, s.metric, c["M"])
    _expect_tile(s, out[4], 17, c["radius"], n_exact=0)
    assert int(out[0][0]) == 300 and (out[2][0] >= 0).all()


# ---- 7: overflow goes to the exact pass ----------------------------------------------------------------------------------------------------
def test_7_overflowing_queries_are_answered_by_the_exact_pass(gpu, stores):
    import torch
    s = stores("overflow")
    c = s.c
    nq = len(c["q"])
    ref = s.reference(c["q"], c["radius"], c["M"])
    out = s.run(c["q"], c["radius"], c["M"])
    _check(out, ref, s.metric, c["M"])
    emitted = _expect_tile(s, out[4], nq, c["radius"], n_exact=None)
    assert 2 <= out[4]["exact"] <= nq // 8, out[4]
    assert (emitted[c["overflow"]] > R.BUFFER).all()
    assert (out[0][c["overflow"]].cpu().numpy() == 5000).all()
    others = np.setdiff1d(np.arange(nq), c["overflow"])
    alone = s.run(c["q"][others], c["radius"], c["M"])
    assert alone[4]["route"] == "tile" and alone[4]["exact"] <= out[4]["exact"] - 2, alone[4]
    sel = _dev(others, gpu)
    assert torch.equal(alone[0], out[0][sel]) and torch.equal(alone[2], out[2][sel])
    assert torch.equal(alone[3].view(torch.int64), out[3][sel].view(torch.int64))    # NaN padding included: the same bits


# ---- 8: nothing and everything ---------------------------------------------------------------------------------------------------------
def test_8_nothing_and_everything(gpu, stores):
    s = stores("nothing")
    c = s.c
    out = s.run(c["q"], c["radius"], c["M"])
    _check(out, s.reference(c["q"], c["radius"], c["M"]), s.metric, c["M"])
    _expect_tile(s, out[4], len(c["q"]), c["radius"], n_exact=0)
    assert int(out[0].abs().sum()) == 0 and int((out[2] != -1).sum()) == 0
    e = R.case("everything")                                                         # the same store, its first 17 queries, radius -inf
    np.testing.assert_array_equal(e["db"], c["db"])
    q = e["q"]
    assert len(q) == 17 and e["radius"] == -np.inf
    out = s.run(q, -np.inf, 64)
    _check(out, s.reference(q, -np.inf, 64), s.metric, 64)
    _expect_tile(s, out[4], 17, -np.inf, n_exact=17)
    assert (out[0].cpu().numpy() == s.idx.ntotal).all()


# ---- 9: the exact route's shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exact_nq3", "exact_dim36", "exact_small_store", "exact_plane_off"])
def test_9_exact_route(gpu, stores, name):
    s = stores(name, **({"hi_plane": 0} if name == "exact_plane_off" else {}))
    c = s.c
    for M in (c["M"], 3):
        ref = s.reference(c["q"], c["radius"], M)
        out = s.run(c["q"], c["radius"], M)
        _check(out, ref, s.metric, M)
        assert out[4] == {"queries": len(c["q"]), "route": "exact", "exact": len(c["q"])}, out[4]
    assert ref[0].max() > 3                                                          # (M = 3 cuts lists: the count stays exact)
    assert ref[0].sum() == sum(len(c["info"]["planted_in"][j]) for j in range(len(c["q"])))


# ---- 10: early abandon on / off ----------------------------------------------------------------------------------------------------------
def test_10_abandon_on_and_off_agree_bit_for_bit(gpu, stores):
    import torch
    on, off = stores("graded_dim128", abandon=1), stores("graded_dim128", abandon=0)
    c = on.c
    ref = on.reference(c["q"], c["radius"], c["M"])
    a = on.run(c["q"], c["radius"], c["M"])
    ab = on.idx.last_abandon()
    b = off.run(c["q"], c["radius"], c["M"])
    print(f"abandon on: {ab}; off: {off.idx.last_abandon()}")
    _check(a, ref, on.metric, c["M"])
    _expect_tile(on, a[4], len(c["q"]), c["radius"])
    assert b[4]["route"] == "tile" and b[4]["exact"] == 0
    assert ab["tasks"] > 0 and off.idx.last_abandon()["tasks"] == 0                  # the one launch took / did not take the ABANDON form
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3].view(torch.int64), b[3].view(torch.int64))


# ---- 11: state -----------------------------------------------------------------------------------------------------------------------------
def test_11_range_calls_leave_the_handle_state_alone(gpu):
    import torch
    s = _Store(gpu, R.case("overflow"))
    c = s.c
    qt = _dev(c["q"], gpu)
    s.idx.search_device(qt, 10, return_f64=True)
    torch.cuda.synchronize()
    D0, I0, K0 = s.idx.search_device(qt, 10, return_f64=True)                        # (consumes the first search's report)
    torch.cuda.synchronize()
    before, cert = s.idx.tuning_info(), s.idx.last_launch()
    assert cert["scan_kind"] == "hi_tile" and cert["certificate"]["queries"] == len(c["q"])
    o7 = s.run(c["q"], c["radius"], c["M"])                                          # case 7: two queries overflow
    o8a = s.run(c["q"], 1.5, c["M"])                                                 # case 8: nothing ...
    o8b = s.run(c["q"][:17], -np.inf, c["M"])                                        # ... and everything
    torch.cuda.synchronize()
    assert o7[4]["exact"] >= 2 and o8a[4]["exact"] == 0 and o8b[4]["exact"] == 17
    assert s.idx.tuning_info() == before
    after = s.idx.last_launch()
    assert after["certificate"] == cert["certificate"] and after["rechecked_queries"] == cert["rechecked_queries"]
    assert s.idx.last_excl_scan()["queries"] == 0
    D1, I1, K1 = s.idx.search_device(qt, 10, return_f64=True)
    assert torch.equal(I0, I1) and torch.equal(D0.view(torch.int32), D1.view(torch.int32)) and torch.equal(K0.view(torch.int64), K1.view(torch.int64))
    # the keys of the range search are the keys the plain search reports
    j = 3                                                                            # (12 rows within the radius: its 10 nearest are among them)
    assert int(o7[0][j]) == 12 and torch.equal(o7[2][j, :10], I1[j])
    np.testing.assert_allclose(o7[3][j, :10].cpu().numpy(), K1[j].cpu().numpy(), rtol=1e-13, atol=0)


# ---- 12: growth and ids --------------------------------------------------------------------------------------------------------------------
def test_12_id_base_and_growth(gpu):
    c = R.case("graded_cosine")
    s = _Store(gpu, c, id_base=1000)
    q = c["q"][:17]
    ref = s.reference(q, c["radius"], c["M"])
    out = s.run(q, c["radius"], c["M"])
    _check(out, ref, s.metric, c["M"])
    _expect_tile(s, out[4], 17, c["radius"])
    I = out[2].cpu().numpy()
    assert I[I >= 0].min() >= 1000
    np.testing.assert_array_equal(np.sort(I[3, :40]), np.sort(c["info"]["planted_in"][3]) + 1000)
    row = int(c["info"]["planted_in"][3][0])
    s.idx.add_device(_dev(np.repeat(s.stored[row:row + 1], 300, axis=0), gpu))
    s.refresh()
    out2 = s.run(q, c["radius"], c["M"])
    _check(out2, s.reference(q, c["radius"], c["M"]), s.metric, c["M"])
    _expect_tile(s, out2[4], 17, c["radius"])
    grown = (out2[0] - out[0]).cpu().numpy()
    assert grown[3] == 300 and grown.sum() == 300


# ---- 13: errors ----------------------------------------------------------------------------------------------------------------------------
def test_13_errors_leave_the_outputs_untouched_and_the_handle_usable(gpu, stores):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    s = stores("graded_cosine")
    c = s.c
    lib = s.idx._lib
    q = _dev(c["q"][:17], gpu)
    M = 8
    cnt = torch.full((17,), -7, dtype=torch.int32, device=gpu)
    D = torch.full((17, M), 123.0, dtype=torch.float32, device=gpu)
    I = torch.full((17, M), -7, dtype=torch.int64, device=gpu)
    st = _lib.stream_ptr(gpu)

    def call(h=None, qp=None, nq=17, radius=0.9, m=M, pc=cnt.data_ptr(), pd=D.data_ptr(), pi=I.data_ptr()):
        return lib.radad_knn_range_search(h if h is not None else s.idx._h, qp if qp is not None else q.data_ptr(), _lib.Q_F32, nq, radius, m,
                                          pc, pd, pi, None, st)
    assert call(m=0) == _lib.RADAD_EINVAL and call(m=_lib.KNN_MAX_K + 1) == _lib.RADAD_EINVAL
    assert call(radius=float("nan")) == _lib.RADAD_EINVAL
    assert call(pc=None) == _lib.RADAD_EINVAL and call(pd=None) == _lib.RADAD_EINVAL and call(pi=None) == _lib.RADAD_EINVAL
    wide = _mk("L2", 16384)                                                          # 16384 * 4 + 96 * 1024 + 16 > 160 KB
    assert call(h=wide._h, m=1024) == _lib.RADAD_EINVAL
    assert call(h=wide._h, m=8) == _lib.RADAD_ESTATE                                 # ... and an empty store
    s.idx.search_begin(q, 5)
    assert call() == _lib.RADAD_EINVAL                                               # a begun search
    s.idx.search_abort()
    assert call(nq=0) == _lib.RADAD_OK
    torch.cuda.synchronize()
    assert (cnt == -7).all() and (D == 123.0).all() and (I == -7).all()
    assert call() == _lib.RADAD_OK                                                   # the handle is usable
    ref = s.reference(c["q"][:17], 0.9, M)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(I.cpu().numpy(), ref[1])


# ---- 14: the Python surface ----------------------------------------------------------------------------------------------------------------
def _config(gpu, tmp_path, index_type, dim=64):
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as Rad
    cfg = Rad.Config()
    cfg.update(device=gpu, feature_dim=dim, tpp_levels=[1], top_k=5, vector_db_index_type=index_type,
               vector_db_path=str(tmp_path / ("vdb_" + index_type)))
    return Rad, cfg


def test_14_vector_database_range_search_batch(gpu, tmp_path, caplog):
    import torch
    Rad, cfg = _config(gpu, tmp_path, "IP")                                          # normalize_for_ip: cosine
    c = R.case("graded_cosine")
    n = len(c["db"])
    vdb = Rad.VectorDatabase(cfg)
    vdb.add_vectors(c["db"], [f"/train/f{i}.wav" for i in range(n)], [i % 2 for i in range(n)], {})
    q = c["q"][:40]
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        lims, D, I, counts = vdb.range_search_batch(q, 0.9, max_per_query=64, return_counts=True)
        assert not [r for r in caplog.records if "max_per_query" in r.getMessage()]
    assert isinstance(lims, np.ndarray) and lims.dtype == np.int64 and lims.shape == (41,) and counts.dtype == np.int32
    np.testing.assert_array_equal(counts, [R.COUNTS[j % 4] for j in range(40)])
    np.testing.assert_array_equal(np.diff(lims), counts)
    assert lims[0] == 0 and len(D) == len(I) == lims[-1] and D.dtype == np.float32 and I.dtype == np.int64
    for j in (1, 2, 3):
        np.testing.assert_array_equal(np.sort(I[lims[j]:lims[j + 1]]), np.sort(c["info"]["planted_in"][j]))
        assert (np.diff(D[lims[j]:lims[j + 1]]) <= 0).all() and (D[lims[j]:lims[j + 1]] > 0.9).all()      # best first
    assert vdb.index.last_range() == {"queries": 40, "route": "tile", "exact": 0}
    # cut to max_per_query: a warning, once, and the exact counts
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        lims2, D2, I2, counts2 = vdb.range_search_batch(q, 0.9, max_per_query=4, return_counts=True)
        assert len([r for r in caplog.records if "max_per_query" in r.getMessage()]) == 1
    np.testing.assert_array_equal(counts2, counts)
    np.testing.assert_array_equal(np.diff(lims2), np.minimum(counts, 4))
    np.testing.assert_array_equal(I2[lims2[3]:lims2[4]], I[lims[3]:lims[3] + 4])
    assert len(vdb.range_search_batch(q, 0.9)) == 3
    # a CUDA tensor in -> CUDA tensors out; one 1-d query
    out = vdb.range_search_batch(_dev(q, gpu), 0.9)
    assert all(t.is_cuda for t in out) and torch.equal(out[0].cpu(), torch.from_numpy(lims))
    l1, d1, i1 = vdb.range_search_batch(q[3], 0.9)
    assert l1.tolist() == [0, 40] and sorted(i1.tolist()) == sorted(c["info"]["planted_in"][3].tolist())
    # an empty store
    empty = Rad.VectorDatabase(cfg)
    empty.create_index(64)
    le, de, ie, ce = empty.range_search_batch(q, 0.9, return_counts=True)
    assert le.tolist() == [0] * 41 and len(de) == len(ie) == 0 and ce.tolist() == [0] * 40


def test_14_ivf_and_sharded_refuse(gpu, tmp_path):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipIVFFlatIndex
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.sharded import ReplicatedSearch, ShardedSearch
    Rad, cfg = _config(gpu, tmp_path, "IVF")
    with pytest.raises(ValueError, match="flat store"):
        HipIVFFlatIndex(64, 64).range_search(np.zeros((1, 64), np.float32), 0.5)
    vdb = Rad.VectorDatabase(cfg)
    vdb.create_index(64)
    with pytest.raises(ValueError, match="flat"):
        vdb.range_search_batch(np.zeros((1, 64), np.float32), 0.5)
    with pytest.raises(ValueError, match="no sharded form"):
        ShardedSearch(None, 0).range_search(None, 0.5)
    with pytest.raises(ValueError, match="no replicated form"):
        ReplicatedSearch(None).range_search(None, 0.5)


def test_14_near_duplicates_finds_a_renamed_copy(gpu, tmp_path):
    Rad, cfg = _config(gpu, tmp_path, "IP")

    class NoExtractor:
        feature_dim = 64

        def extract_features(self, segments):
            raise AssertionError("not used")
    pipe = Rad.HotPathPipeline(cfg, feature_extractor=NoExtractor())
    c = R.case("graded_cosine")
    n = len(c["db"])
    paths = [f"/train/f{i}.wav" for i in range(n)]
    own, renamed = (int(r) for r in c["info"]["planted_in"][2][:2])                  # two of query 2's five near-copies
    paths[own] = "/train/vocoder3/clip2.wav"
    paths[renamed] = "/train/renamed_copy.wav"
    labels = [i % 2 for i in range(n)]
    pipe.vector_db.add_vectors(c["db"], paths, labels, {})
    q = c["q"][:20]
    query_paths = [f"/eval/clip{j}.wav" for j in range(20)]
    plain = pipe.near_duplicates(q, 0.9)
    assert [len(h) for h in plain] == [R.COUNTS[j % 4] for j in range(20)]
    assert {h[0] for h in plain[2]} == {paths[int(r)] for r in c["info"]["planted_in"][2]}
    assert all(h[1] == labels[paths.index(h[0])] and h[2] > 0.9 for h in plain[2])
    assert [h[2] for h in plain[3]] == sorted((h[2] for h in plain[3]), reverse=True)
    audit = pipe.near_duplicates(_dev(q, gpu), 0.9, query_paths=query_paths)
    got = {h[0] for h in audit[2]}
    assert "/train/vocoder3/clip2.wav" not in got and "/train/renamed_copy.wav" in got and len(audit[2]) == 4
    assert [len(h) for j, h in enumerate(audit) if j != 2] == [len(h) for j, h in enumerate(plain) if j != 2]
    assert os.path.basename(paths[own]) == os.path.basename(query_paths[2])
