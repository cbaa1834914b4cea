"""Exclusion-aware flat search (radad_knn_search_excl / HipFlatIndex.search_excluding): the exact top-k among the rows whose tag is
not excluded, however many excluded rows precede them.  The reference searches K + 10 rows, drops the excluded hits and pads
(pipeline.py:478,491-515); that stays the default (radad_filter_topk) and pads a query whose neighbourhood is crowded with excluded
rows although admissible neighbours exist.

Reference (tests/exclusion_ref.py, checked on the CPU by tests/test_exclusion_reference.py): the float64 oracle over the admissible
rows AS STORED, ids remapped.  The number of queries that take the exact pass is derived from the oracle's top-k_fetch over the whole
store and asserted with equality: every id of the fast pass is exact.  Distances: the tolerances of tests/test_gpu_knn.py (1e-4
absolute on unit-norm data, 1e-6 on raw L2)."""
import numpy as np
import pytest

from exclusion_ref import crowded, expected_exact, expected_excluding

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


class _Case:
    """a store on the device, its rows as stored, tags and exclusion set"""

    def __init__(self, gpu, metric, db, q, tags, excl, f16=False, id_base=0):
        self.metric, self.q, self.tags, self.excl, self.gpu = metric, q, np.asarray(tags, np.int64), excl, gpu
        self.idx = _mk(metric, db.shape[1], f16, id_base)
        self.idx.add(db)
        self.stored = _stored(self.idx, len(db), gpu)
        self.tags_t = _dev(self.tags, gpu)
        self.excl_t = None if excl is None else _dev(np.asarray(excl, np.int64), gpu)

    def run(self, k, k_fetch, nq=None, q=None, q_ref=None, return_f64=False):
        """search the first nq queries, compare with the reference, assert the derived exact-pass count; -> that count"""
        q = self.q[:nq] if q is None else q
        q_ref = (q if isinstance(q, np.ndarray) else None) if q_ref is None else q_ref
        qt = _dev(q, self.gpu) if isinstance(q, np.ndarray) else q
        out = self.idx.search_excluding(qt, k, self.tags_t, self.excl_t, k_fetch=k_fetch, return_f64=return_f64)
        ed, ei = expected_excluding(self.stored, self.tags, self.excl, q_ref, k, self.metric, self.idx.id_base)
        want = int(expected_exact(self.stored, self.tags, self.excl, q_ref, k, k_fetch, self.metric).sum())
        info = self.idx.last_excl()
        print(f"exact pass: {info['exact']} of {info['queries']} queries (derived {want}), scan {self.idx.last_launch()['scan_kind']}")
        _check(out[0], out[1], ed, ei, self.metric, out[2] if return_f64 else None)
        assert info == {"queries": len(q_ref), "exact": want}, (info, want)
        return want


# ---- 1. crowded neighbourhoods: the default path pads, the exclusion-aware search does not ----------------------------------------
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_crowded_neighbourhoods(gpu, metric):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    db, q, tags, excl, which = crowded(20000, 64, 40, 12, 30, 9101)
    c = _Case(gpu, metric, db, q, tags, excl)
    n_exact = c.run(5, 15, return_f64=True)
    assert n_exact >= 12
    # the contrast: the same data through the K + 10 over-fetch and radad_filter_topk
    D15, I15 = c.idx.search_device(_dev(q, gpu), 15)
    fd = torch.empty((40, 5), device=gpu)
    fi = torch.empty((40, 5), device=gpu, dtype=torch.int64)
    _lib.check(_lib.load().radad_filter_topk(D15.data_ptr(), I15.data_ptr(), 40, 15, 5, c.tags_t.data_ptr(), 20000, 0,
                                             c.excl_t.data_ptr(), c.excl_t.numel(), fd.data_ptr(), fi.data_ptr(), 0, _lib.stream_ptr(gpu)))
    fd, fi = fd.cpu().numpy(), fi.cpu().numpy()
    assert np.all(fi[which] == -1) and np.all(np.isnan(fd[which]))               # 30 excluded near-duplicates fill all 15 hits
    D, I = c.idx.search_excluding(_dev(q, gpu), 5, c.tags_t, c.excl_t, k_fetch=15)
    assert np.all(I.cpu().numpy()[which] >= 0)
    rest = np.setdiff1d(np.arange(40), which)
    full = (fi[rest] >= 0).all(axis=1)                                           # where the over-fetch sufficed both agree
    np.testing.assert_array_equal(I.cpu().numpy()[rest][full], fi[rest][full])


# ---- 2. every fast-pass route ------------------------------------------------------------------------------------------------------
_ROUTES = {"dense": (4096, 64, "L2", False), "hi_plane": (20000, 64, "COSINE", False), "fp32": (20000, 36, "L2", False),
           "f16_store": (20000, 64, "L2", True)}


@pytest.fixture(scope="module")
def route_cases(gpu):
    cache = {}

    def get(name):
        if name not in cache:
            n, dim, metric, f16 = _ROUTES[name]
            db, q, tags, excl, _ = crowded(n, dim, 300, 100, 30, 9200 + len(cache))
            cache[name] = _Case(gpu, metric, db, q, tags, excl, f16=f16)
        return cache[name]
    yield get
    cache.clear()


@pytest.mark.parametrize("k_fetch", [5, 15, 200])
@pytest.mark.parametrize("nq", [1, 16, 17, 300])
@pytest.mark.parametrize("route", ["dense", "hi_plane", "fp32", "f16_store"])
def test_fast_pass_routes(gpu, route_cases, route, nq, k_fetch):
    c = route_cases(route)
    n_exact = c.run(5, k_fetch, nq=nq)
    kind = c.idx.last_launch()["scan_kind"]
    if k_fetch == 200:
        assert n_exact == 0                                           # 30 duplicates + 64 excluded rows leave >= 106 of 200 hits
        assert kind == ("f32_dense" if route == "dense" else "f32_tile"), kind      # above 128: no f16 scan
    else:
        assert n_exact >= (nq + 2) // 3                               # queries 0, 3, 6, ... are crowded
    if route == "dense":
        assert kind == "f32_dense", kind
    if route == "hi_plane" and k_fetch <= 15:
        assert kind == ("hi_tile" if nq > 16 else "hi_smallq"), kind
    if route == "fp32":
        assert kind == "f32_tile", kind


def test_bf16_queries(gpu, route_cases):
    import torch
    c = route_cases("hi_plane")
    qb = torch.from_numpy(c.q[:40]).to(gpu).bfloat16()
    assert c.run(5, 15, q=qb, q_ref=qb.float().cpu().numpy()) >= 1


# ---- 3. more listed queries than one launch group; lists of the exact pass beyond one strip ----------------------------------------
def test_many_listed_queries(gpu, route_cases):
    assert route_cases("fp32").run(5, 15) >= 100


@pytest.mark.parametrize("k,k_fetch", [(64, 80), (100, 128)])
def test_listed_queries_long_lists(gpu, k, k_fetch):
    db, q, tags, excl, which = crowded(20000, 64, 300, 40, 100, 9301)
    c = _Case(gpu, "L2", db, q, tags, excl)
    assert c.run(k, k_fetch) >= 40


# ---- 3b. the two forms of the compaction kernel agree at the strip boundaries of its walk ---------------------------------------------
@pytest.fixture(scope="module")
def strip_case(gpu):
    # 62 excluded near-duplicates in front of each crowded query: its admissible hits start at position 62 of the fast-pass list and
    # run across the end of the first strip of 64 (k_fetch 64: two of them, 65: three, 200: all five, the fifth in the second strip)
    db, q, tags, excl, which = crowded(20000, 64, 40, 12, 62, 9351)
    c = _Case(gpu, "L2", db, q, tags, excl)
    c.want = expected_excluding(c.stored, c.tags, c.excl, q, 5, "L2")
    yield c


@pytest.mark.parametrize("k_fetch", [5, 15, 64, 65, 200])
def test_compaction_forms_agree_at_strip_boundaries(gpu, strip_case, k_fetch):
    """k_excl_compact<false> (search_excluding) and k_excl_compact<true> (search_excluding_begin) share one walk: the rows the shard
    form leaves (finish without flags) are the whole-store form's bit for bit for every query that form did not list, the full
    call is the oracle's answer for every query, and the frontier is the model's (tests/sharded_excl_ref.shard_begin).  L2: the
    float64 keys of the excluded near-duplicates a frontier may be are then apart by far more than their rounding, so the frontier
    ID is compared exactly; its key and the distances with this file's L2 tolerance (summation order differs from the oracle's)."""
    import torch
    from sharded_excl_ref import shard_begin
    c, k = strip_case, 5
    qt = _dev(c.q, gpu)
    listed = expected_exact(c.stored, c.tags, c.excl, c.q, k, k_fetch, "L2")
    D, I, K64 = c.idx.search_excluding(qt, k, c.tags_t, c.excl_t, k_fetch=k_fetch, return_f64=True)
    info = c.idx.last_excl()
    Kb, Ib, FK, FI = c.idx.search_excluding_begin(qt, k, c.tags_t, c.excl_t, k_fetch)
    Df, If, Kf = c.idx.search_excluding_finish(None, return_f64=True)
    print(f"k_fetch {k_fetch}: listed {info['exact']} of {info['queries']} (derived {int(listed.sum())})")
    assert info == {"queries": 40, "exact": int(listed.sum())}, info
    assert (k_fetch == 200) == (not listed.any())                     # the twelve crowded queries are listed unless all five fit
    _check(D, I, c.want[0], c.want[1], "L2", K64)
    keep = torch.from_numpy(~listed).to(gpu)
    assert torch.equal(If[keep], I[keep])
    assert torch.equal(Df[keep].view(torch.int32), D[keep].view(torch.int32))
    assert torch.equal(Kf[keep].view(torch.int64), K64[keep].view(torch.int64))
    mk, mi, mfk, mfi = shard_begin(c.stored, c.tags, c.excl, c.q, k, k_fetch, "L2")
    np.testing.assert_array_equal(Ib.cpu().numpy(), mi)
    np.testing.assert_array_equal(If.cpu().numpy(), mi)
    fk, fi = FK.cpu().numpy(), FI.cpu().numpy()
    np.testing.assert_array_equal(fi, mfi)
    assert np.all(fi >= 0)                                            # 20 000 rows: something is always unseen
    np.testing.assert_allclose(fk, mfk, rtol=1e-6, atol=1e-6)
    full = mi[:, -1] >= 0
    np.testing.assert_array_equal(fk[full].view(np.int64), Kb.cpu().numpy()[full, -1].view(np.int64))   # the k-th survivor itself


# ---- 4. few admissible rows ------------------------------------------------------------------------------------------------------------
def test_few_admissible_rows(gpu):
    db, q, tags, _, _ = crowded(4096, 64, 24, 4, 10, 9401)
    keep = np.array([5, 1700, 4095])
    c = _Case(gpu, "L2", db, q, tags, np.unique(np.delete(tags, keep)))
    assert c.run(5, 15, return_f64=True) == 24
    D, I = c.idx.search_excluding(_dev(q, gpu), 5, c.tags_t, c.excl_t, k_fetch=15)
    I = I.cpu().numpy()
    assert np.all(np.sort(I[:, :3], axis=1) == keep) and np.all(I[:, 3:] == -1) and np.all(np.isnan(D.cpu().numpy()[:, 3:]))


def test_store_smaller_than_k_fetch(gpu):
    db, q, tags, _, _ = crowded(8, 64, 24, 0, 0, 9402, extra_excl=0)
    c = _Case(gpu, "L2", db, q, tags, np.unique(tags[[0, 2, 3, 5, 6]]))
    assert c.run(5, 15, return_f64=True) == 0                         # the list is all the store has: proved, 3 ids then -1 / NaN
    c3 = _Case(gpu, "COSINE", db[:3], q, tags[:3], tags[1:2])         # fewer rows than k
    assert c3.run(5, 15) == 0


# ---- 5. nothing excluded ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 40])
def test_no_exclusion_is_the_plain_search(gpu, route_cases, nq):
    import torch
    c = route_cases("hi_plane")
    qt = _dev(c.q[:nq], gpu)
    D0, I0 = c.idx.search_device(qt, 5)
    for excl in (None, torch.empty(0, dtype=torch.int64, device=gpu)):
        D, I, K64 = c.idx.search_excluding(qt, 5, c.tags_t, excl, k_fetch=15, return_f64=True)
        assert c.idx.last_excl() == {"queries": nq, "exact": 0}
        assert torch.equal(I, I0) and torch.equal(D, D0) and torch.equal(K64.float(), D0)
    D, I = c.idx.search_excluding(qt, 5, None, None)                 # k_fetch = k + 10 by default, no tags needed
    assert torch.equal(I, I0) and torch.equal(D, D0)


# ---- 6. shared tags and ties -------------------------------------------------------------------------------------------------------------
def test_shared_tags(gpu):
    n = 20000
    db, q, tags, excl, which = crowded(n, 64, 40, 12, 30, 9601, tags=np.arange(n) // 4 + 3)
    c = _Case(gpu, "L2", db, q, tags, excl)
    assert np.isin(tags, excl).sum() == 4 * len(excl)                # all four rows of a dropped tag go
    assert c.run(5, 15) >= 12


def test_bit_identical_rows_come_in_id_order(gpu):
    db, q, tags, _, _ = crowded(20000, 64, 17, 0, 0, 9602, extra_excl=0)
    rows = np.sort(np.random.default_rng(9603).choice(20000, 50, replace=False))
    db[rows] = q[0] + np.float32(1e-3)                                # 50 bit-identical rows at rank 1 of query 0
    c = _Case(gpu, "L2", db, q, tags, np.unique(tags[rows[1::2]]))    # every second one excluded
    assert c.run(30, 40) >= 1                                         # 40 hits = 40 of the 50: 20 survivors < 30
    D, I = c.idx.search_excluding(_dev(q, gpu), 30, c.tags_t, c.excl_t, k_fetch=40)
    np.testing.assert_array_equal(I.cpu().numpy()[0, :25], rows[0::2])
    assert c.run(10, 40) == 0                                         # ... and in id order from the fast pass too
    D, I = c.idx.search_excluding(_dev(q, gpu), 10, c.tags_t, c.excl_t, k_fetch=40)
    np.testing.assert_array_equal(I.cpu().numpy()[0], rows[0::2][:10])


# ---- 7. id_base ------------------------------------------------------------------------------------------------------------------------
def test_id_base(gpu):
    db, q, tags, excl, which = crowded(20000, 64, 40, 12, 30, 9701)
    c = _Case(gpu, "COSINE", db, q, tags, excl, id_base=1000)
    assert c.run(5, 15) >= 12
    D, I = c.idx.search_excluding(_dev(q, gpu), 5, c.tags_t, c.excl_t, k_fetch=15)
    I = I.cpu().numpy()
    assert I.min() >= 1000 and not np.isin(tags[I - 1000], excl).any()


# ---- 8. the training_file_ids shape: most of the store is excluded -----------------------------------------------------------------------
def test_most_of_the_store_excluded(gpu):
    db, q, tags, _, _ = crowded(4096, 64, 24, 0, 0, 9801, extra_excl=0)
    gone = np.random.default_rng(9802).choice(4096, 3900, replace=False)
    c = _Case(gpu, "COSINE", db, q, tags, np.unique(tags[gone]))
    assert c.run(5, 15) == 24                                         # every query takes the exact pass


# ---- 9. arguments ------------------------------------------------------------------------------------------------------------------------
def test_arguments(gpu, route_cases):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    c = route_cases("hi_plane")
    qt = _dev(c.q[:20], gpu)
    D0, I0 = c.idx.search_device(qt, 5)
    with pytest.raises(ValueError):
        c.idx.search_excluding(qt, 5, c.tags_t, c.excl_t, k_fetch=4)
    with pytest.raises(ValueError):
        c.idx.search_excluding(qt, 1025, c.tags_t, c.excl_t, k_fetch=1025)
    with pytest.raises(ValueError):
        c.idx.search_excluding(qt, 0, c.tags_t, c.excl_t, k_fetch=15)
    with pytest.raises(ValueError):
        c.idx.search_excluding(qt, 5, c.tags_t, c.excl_t, k_fetch=1025)
    D = torch.empty((20, 5), device=gpu)
    I = torch.empty((20, 5), device=gpu, dtype=torch.int64)
    with pytest.raises(ValueError):                                   # an exclusion set of 3 tags that is not there
        _lib.check(_lib.load().radad_knn_search_excl(c.idx._h, qt.data_ptr(), _lib.Q_F32, 20, 5, 15, c.tags_t.data_ptr(), None, 3,
                                                     D.data_ptr(), I.data_ptr(), None, _lib.stream_ptr(gpu)))
    with pytest.raises(ValueError):                                   # ... or without the row tags
        _lib.check(_lib.load().radad_knn_search_excl(c.idx._h, qt.data_ptr(), _lib.Q_F32, 20, 5, 15, None, c.excl_t.data_ptr(), 3,
                                                     D.data_ptr(), I.data_ptr(), None, _lib.stream_ptr(gpu)))
    c.idx.search_begin(qt, 5)
    with pytest.raises(ValueError):                                   # a begun search owns the handle
        c.idx.search_excluding(qt, 5, c.tags_t, c.excl_t, k_fetch=15)
    c.idx.search_abort()
    empty = _mk("L2", 64)
    with pytest.raises(ValueError):                                   # an empty store
        empty.search_excluding(qt, 5, None, None)
    D1, I1 = c.idx.search_device(qt, 5)                               # after the refused calls a plain search still works
    assert torch.equal(I1, I0) and torch.equal(D1, D0)
    c.run(5, 15, nq=20)


# ---- 10. state isolation -------------------------------------------------------------------------------------------------------------------
def test_state_describes_the_fast_pass_only(gpu):
    import torch
    db, q, tags, excl, which = crowded(20000, 64, 300, 100, 30, 9901)
    c = _Case(gpu, "L2", db, q, tags, excl)
    qt = _dev(q, gpu)
    D0, I0 = c.idx.search_device(qt, 5)
    torch.cuda.synchronize()
    c.idx.search_device(qt, 15)
    plain = c.idx.last_launch()
    torch.cuda.synchronize()
    c.idx.search_device(qt, 5)                                        # (consumes the report of the k = 15 search)
    before = c.idx.tuning_info()
    assert c.run(5, 15) >= 100                                        # a third of the batch takes the exact pass ...
    torch.cuda.synchronize()
    info = c.idx.last_launch()
    assert info["scan_kind"] == plain["scan_kind"] and info["certificate"]["queries"] == 300, (info, plain)
    assert info["certificate"]["rejected"] == plain["certificate"]["rejected"] < 100, (info, plain)
    D1, I1 = c.idx.search_device(qt, 5)
    after = c.idx.tuning_info()
    # ... and leaves ONE report, the fast pass's (nothing rejected): no retuning follows
    assert after["reports_consumed"] - before["reports_consumed"] <= 2, (before, after)
    assert after["cap_boost"] == before["cap_boost"] and after["fp32_searches_left"] == before["fp32_searches_left"]
    assert torch.equal(I1, I0) and torch.equal(D1, D0)
